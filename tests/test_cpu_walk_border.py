"""The wave walk of hpmvs_amd/frontier.py (`_walk`) with BORDER candidates and the pre-occupied refusal key of the real-tree
level calls (extend_level_tree), without a device: the toy of tests/test_cpu_frontier_walk.py with two additions.

  * A refined candidate is a border candidate with probability 0.2 (CellProcessor.cpp:147-153: it passed every gate but lies
    outside the root): in the sequential loop it reads the maps like any other, gets stage 27 after the three counts, writes
    nothing and occupies nothing.  Its post_key is a key nothing else holds, as _TreeKeys gives it.
  * post_key is REFUSED (0) with probability 0.1 -- addConditional would refuse on the tree as the level found it -- and 0 is
    in `occupied` from the start: stage 26.  A pre_key is unique ("outside") with probability 0.1: never occupied.

Every queue needs at least 2 waves, accepts at least one candidate and -- over the seeds -- border candidates are deferred behind
a write they read: dropping the reads check for them, letting them write, or letting them occupy their key fails the test.
Without `border` the walk is the one tests/test_cpu_frontier_walk.py pins (the default argument)."""
import random

import pytest

from hpmvs_amd.frontier import REFUSED, _walk

MIN = 3
N_CELLS, N_KEYS, N_CAND = 40, 30, 60
FAIL = 1


def _toy(seed, with_events):
    r = random.Random(seed)
    R, W, pre, post, ref, thr, ev, queue, border = {}, {}, {}, {}, {}, {}, [], [], set()
    for t in range(N_CAND):
        if with_events and r.random() < 0.3:
            queue.append(("e", len(ev)))
            ev.append({r.randrange(N_CELLS) for _ in range(r.randint(1, 3))})
        R[t] = {r.randrange(N_CELLS) for _ in range(r.randint(1, 5))}
        W[t] = {r.randrange(N_CELLS) for _ in range(r.randint(1, 3))}
        pre[t] = ("outside", t) if r.random() < 0.1 else 1 + r.randrange(N_KEYS)
        ref[t] = r.random() < 0.85
        u = r.random()
        if ref[t] and u < 0.2:
            border.add(t)
            post[t] = ("border", t)
        else:
            post[t] = REFUSED if u < 0.3 else 1 + r.randrange(N_KEYS)
        queue.append(("c", t))
    occ0 = {REFUSED} | {1 + r.randrange(N_KEYS) for _ in range(4)}
    maps0 = {c: r.randrange(2) for c in range(N_CELLS)}
    for t in range(N_CAND):
        thr[t] = r.randint(1, 4)
    return R, W, pre, post, ref, thr, ev, queue, occ0, maps0, border


def _run(seed, with_events, flags):
    R, W, pre, post, ref, thr, ev, queue, occ0, maps0, border = _toy(seed, with_events)
    nimg = {t: 4 for t in range(N_CAND)}

    def count(maps, t):
        s = sum(maps[c] for c in R[t])
        return (MIN if s < thr[t] else 0, MIN if s == 0 and len(R[t]) > 3 else 0, 4 if s != 1 else 2)

    def do(maps, kind, t):
        for c in (ev[t] if kind == "e" else W[t]):
            maps[c] = 0 if kind == "e" else maps[c] + 1

    # the sequential loop
    maps, occ, st, acc, cnt = dict(maps0), set(occ0), {t: FAIL for t in range(N_CAND)}, [], {}
    written = set()           # cells written so far by this level: a border candidate reading one depends on the order
    late_border = 0
    for kind, t in queue:
        if kind == "e":
            do(maps, kind, t)
            written |= ev[t]
        elif pre[t] in occ:
            st[t] = 20
        elif ref[t]:
            v, b, f = cnt[t] = count(maps, t)
            if not v >= MIN:
                st[t] = 23
            elif not b < MIN:
                st[t] = 24
            elif not (f >= MIN - 1 and f / nimg[t] > 0.75):
                st[t] = 25
            elif t in border:
                st[t] = 27
                late_border += bool(R[t] & written)
            elif post[t] in occ:
                st[t] = 26
            else:
                occ.add(post[t]); st[t] = 0; acc.append(t); do(maps, kind, t)
                written |= W[t]
    # the walk
    maps2, occ2, st2, cnt2 = dict(maps0), set(occ0), {t: FAIL for t in range(N_CAND)}, {}
    arg = border if not flags else [t in border for t in range(N_CAND)]
    accepted, waves, deferred = _walk(queue, pre, post, ref, nimg, R.__getitem__, W.__getitem__, ev, occ2, MIN, st2, cnt2,
                                      lambda todo: [count(maps2, t) for t in todo], lambda ops: [do(maps2, k, t) for k, t in ops],
                                      border=arg)
    assert st2 == st and sorted(accepted) == acc and occ2 == occ and maps2 == maps, (seed, with_events)
    assert {t: c for t, c in cnt2.items() if c != (-1, -1, -1)} == cnt, (seed, with_events)     # counts at decision time
    assert not any(isinstance(k, tuple) for k in occ2)                                          # a border key is never occupied
    assert len(deferred) == waves and deferred[-1] == 0
    assert waves >= 2 and len(acc) >= 1, (seed, with_events, waves, len(acc))
    return waves, set(st.values()), sum(1 for t in border if st[t] == 27), late_border


@pytest.mark.parametrize("with_events", [False, True])
def test_walk_with_border_candidates_equals_the_sequential_loop(with_events):
    res = [_run(seed, with_events, flags=bool(seed & 1)) for seed in range(500)]
    stages = set().union(*(s for _, s, _, _ in res))
    assert {0, FAIL, 20, 23, 24, 25, 26, 27} <= stages, stages
    assert sum(b for _, _, b, _ in res) >= 500 and sum(l for _, _, _, l in res) >= 100
    print(f"events {with_events}: waves {min(w for w, *_ in res)} .. {max(w for w, *_ in res)}, stage 27: {sum(b for _, _, b, _ in res)}, "
          f"of them behind a write they read: {sum(l for _, _, _, l in res)}")


def test_default_border_argument_changes_nothing():
    """border = None and an empty set give the walk without border candidates: same stages, same waves."""
    R, W, pre, post, ref, thr, ev, queue, occ0, maps0, _ = _toy(3, True)
    out = []
    for arg in ({}, {"border": None}, {"border": set()}):
        maps, st = dict(maps0), {t: FAIL for t in range(N_CAND)}

        def do(ops):
            for kind, t in ops:
                for c in (ev[t] if kind == "e" else W[t]):
                    maps[c] = 0 if kind == "e" else maps[c] + 1

        acc, waves, deferred = _walk(queue, pre, post, ref, {t: 4 for t in range(N_CAND)}, R.__getitem__, W.__getitem__, ev, set(occ0),
                                     MIN, st, {}, lambda todo: [(MIN, 0, 4) if sum(maps[c] for c in R[t]) < thr[t] else (0, 0, 4) for t in todo],
                                     do, **arg)
        out.append((acc, waves, deferred, st, maps))
    assert out[0] == out[1] == out[2] and 27 not in out[0][3].values()
