"""What the level-walk tests share (tests/test_cpu_level_walk.py, tests/test_gpu_level_walk.py):
  * the flag bits of hpmvs_level_walk_batch and HostWalk, hpmvs_amd/csrc/level_walk.hpp's walk_by_rounds compiled by g++
    (tests/level_walk_host.cpp) with its device behind two Python callbacks;
  * toy(): the toy queues of tests/test_cpu_frontier_walk.py, widened with two to four key sets, border candidates, candidates
    without a pre key and leaves taken when the level starts;
  * graph_of(): the conflict graph of a queue from its read / write cell sets, by the definition of conflicts.hpp;
  * run_walk() / run_rounds(): one queue through frontier._walk and through the restatement, each returning the same record."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

from hpmvs_amd.frontier import _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "level_walk_host.cpp")
EVENT, REFINED, BORDER, HAS_PRE, PRE_TAKEN, POST_TAKEN = 1, 2, 4, 8, 16, 32
MIN = 3
FAIL = 1    # the stage of a candidate that was not refined


class HostWalk:
    GATES = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    APPLY = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_int32), C.c_int)

    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "liblevel_walk_host.so")
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.lw_walk.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 15 + [self.GATES, self.APPLY]

    def walk(self, flags, sets, pre, post, graph, n_images, stage, gates, apply, min_images=MIN):
        """gates(items) -> [(v, b, f)], apply(items, any_event).  Returns (rc, stage, counts, accepted, wave, n_waves, rounds)."""
        n = len(flags)
        flags = np.ascontiguousarray(flags, np.uint8); pre = np.ascontiguousarray(pre, np.uint64); post = np.ascontiguousarray(post, np.uint64)
        sets = None if sets is None else np.ascontiguousarray(sets, np.int32)
        fo, fa, ao, aa = [np.ascontiguousarray(a, np.uint32) for a in graph]
        ni = np.ascontiguousarray(n_images, np.int32)
        st = np.ascontiguousarray(stage, np.int32).copy()
        counts = np.full((n, 3), 7, np.int32); acc = np.full(n, 7, np.uint8); wave = np.full(n, 7, np.int32)
        rounds = np.zeros(max(n, 1), np.int32)
        nw = C.c_int32(-1)

        def g(count, items, vbf):
            for k, c in enumerate(gates([items[k] for k in range(count)])):
                vbf[3 * k], vbf[3 * k + 1], vbf[3 * k + 2] = c

        rc = self.L.lw_walk(n, min_images, flags.ctypes.data, None if sets is None else sets.ctypes.data, pre.ctypes.data, post.ctypes.data,
                            fo.ctypes.data, fa.ctypes.data, ao.ctypes.data, aa.ctypes.data, ni.ctypes.data, st.ctypes.data,
                            counts.ctypes.data, acc.ctypes.data, wave.ctypes.data, C.addressof(nw), rounds.ctypes.data, self.GATES(g),
                            self.APPLY(lambda count, items, ev: apply([items[k] for k in range(count)], bool(ev))))
        return rc, st, counts, acc, wave, nw.value, rounds[:max(nw.value, 0)].tolist()


def csr(lists):
    off = np.zeros(len(lists) + 1, np.uint32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([j for l in lists for j in l], np.uint32)


def graph_of(nodes, R, W, ev):
    """conflicts.hpp's lists over `nodes` (queue items ("e", j) / ("c", t), the events and the refined candidates) from the cell
    sets: a candidate reads R[t] and writes W[t], an event writes ev[j] and reads nothing."""
    wr = [ev[t] if kind == "e" else W[t] for kind, t in nodes]
    rd = [set() if kind == "e" else R[t] for kind, t in nodes]
    is_ev = [kind == "e" for kind, _ in nodes]
    flow, anti = [], []
    for i in range(len(nodes)):
        if is_ev[i]:
            flow.append([j for j in range(i) if not is_ev[j] and wr[j] & wr[i]])
            anti.append([j for j in range(i) if not is_ev[j] and rd[j] & wr[i]])
        else:
            flow.append([j for j in range(i) if wr[j] & rd[i]])
            anti.append([j for j in range(i) if (wr[j] & wr[i] if is_ev[j] else rd[j] & wr[i])])
    return csr(flow) + csr(anti)


class Toy:
    """One queue: per candidate t read cells R[t], write cells W[t], key set, pre / post key (None: no pre key), refined, border, a
    threshold; events ev[j] (cell sets); queue items; occ0: the (set, key) leaves taken at the start; maps0."""

    def __init__(self, seed, with_events, n_cand=60, n_cells=40, n_keys=10):
        r = random.Random(seed)
        self.n_cand, self.n_sets = n_cand, r.randint(2, 4)
        self.R, self.W, self.set, self.pre, self.post, self.ref, self.border, self.thr = {}, {}, {}, {}, {}, {}, {}, {}
        self.ev, self.queue = [], []
        for t in range(n_cand):
            if with_events and r.random() < 0.3:
                self.queue.append(("e", len(self.ev)))
                self.ev.append({r.randrange(n_cells) for _ in range(r.randint(1, 3))})
            self.R[t] = {r.randrange(n_cells) for _ in range(r.randint(1, 5))}
            self.W[t] = {r.randrange(n_cells) for _ in range(r.randint(1, 3))}
            self.set[t] = r.randrange(self.n_sets)
            self.pre[t] = r.randrange(n_keys) if r.random() < 0.9 else None
            self.post[t] = r.randrange(n_keys)
            self.ref[t] = r.random() < 0.85
            self.border[t] = self.ref[t] and r.random() < 0.12
            self.queue.append(("c", t))
        self.occ0 = {(r.randrange(self.n_sets), r.randrange(n_keys)) for _ in range(5)}
        self.maps0 = {c: r.randrange(2) for c in range(n_cells)}
        for t in range(n_cand):
            self.thr[t] = r.randint(1, 4)

    def count(self, maps, t):
        s = sum(maps[c] for c in self.R[t])
        return (MIN if s < self.thr[t] else 0, MIN if s == 0 and len(self.R[t]) > 3 else 0, 4 if s != 1 else 2)

    def do(self, maps, kind, t):
        for c in (self.ev[t] if kind == "e" else self.W[t]):
            maps[c] = 0 if kind == "e" else maps[c] + 1


def run_walk(T):
    """frontier._walk over the toy.  Returns the record both runs are compared by and what only the host walk can tell:
    (record, event_deferred)."""
    n = T.n_cand
    maps, occ = dict(T.maps0), set(T.occ0)
    st, cnt = {t: FAIL for t in range(n)}, {}
    pre = {t: (T.set[t], T.pre[t]) if T.pre[t] is not None else ("outside", t) for t in range(n)}
    post = {t: None if not T.ref[t] else ("border", t) if T.border[t] else (T.set[t], T.post[t]) for t in range(n)}
    calls = {"gates": 0, "late_event": False}

    def gates(todo):
        calls["gates"] += 1
        return [T.count(maps, t) for t in todo]

    def apply(ops):
        if calls["gates"] >= 2 and any(k == "e" for k, _ in ops):
            calls["late_event"] = True     # (applied after a second gate pass: it was deferred in wave 1)
        for k, t in ops:
            T.do(maps, k, t)

    accepted, waves, deferred = _walk(T.queue, pre, post, T.ref, {t: 4 for t in range(n)}, T.R.__getitem__, T.W.__getitem__, T.ev, occ,
                                      MIN, st, cnt, gates, apply, border={t for t in range(n) if T.border[t]})
    counts = {t: tuple(cnt.get(t, (-1, -1, -1))) for t in range(n)}
    return (st, counts, accepted, waves, deferred, occ, maps), calls["late_event"]


def toy_items(T):
    """The queue as hpmvs_level_walk_batch takes it: (flags, set, pre, post, stage, nodes)."""
    flags, sets, pre, post, stage, nodes = [], [], [], [], [], []
    for kind, t in T.queue:
        if kind == "e":
            flags.append(EVENT); sets.append(0); pre.append(0); post.append(0); stage.append(0)
            nodes.append((kind, t))
            continue
        f = (REFINED if T.ref[t] else 0) | (BORDER if T.border[t] else 0)
        if T.pre[t] is not None:
            f |= HAS_PRE | (PRE_TAKEN if (T.set[t], T.pre[t]) in T.occ0 else 0)
        if T.ref[t] and not T.border[t] and (T.set[t], T.post[t]) in T.occ0:
            f |= POST_TAKEN
        flags.append(f); sets.append(T.set[t]); pre.append(T.pre[t] if T.pre[t] is not None else 0); post.append(T.post[t])
        stage.append(FAIL)
        if T.ref[t]:
            nodes.append((kind, t))
    return flags, sets, pre, post, stage, nodes


def run_rounds(host, T):
    """The restatement over the toy.  Returns (record, rounds per wave)."""
    flags, sets, pre, post, stage, nodes = toy_items(T)
    maps = dict(T.maps0)
    q = T.queue

    def apply(items, any_event):
        assert any_event == any(q[i][0] == "e" for i in items) and items == sorted(items)
        for i in items:
            T.do(maps, *q[i])

    rc, st, counts, acc, wave, n_waves, rounds = host.walk(flags, sets, pre, post, graph_of(nodes, T.R, T.W, T.ev), [4] * len(q), stage,
                                                           lambda items: [T.count(maps, q[i][1]) for i in items], apply)
    assert rc == 0, rc
    cand = [(i, t) for i, (kind, t) in enumerate(q) if kind == "c"]
    accepted = [t for w, i, t in sorted((wave[i], i, t) for i, t in cand if acc[i])]
    occ = set(T.occ0) | {(T.set[t], T.post[t]) for t in accepted}
    deferred = [int((wave > w + 1).sum()) for w in range(n_waves)]
    assert wave.min() >= 1 and not acc[[i for i, (kind, _) in enumerate(q) if kind == "e"]].any()
    return ({t: int(st[i]) for i, t in cand}, {t: tuple(int(c) for c in counts[i]) for i, t in cand}, accepted, n_waves, deferred, occ,
            maps), rounds
