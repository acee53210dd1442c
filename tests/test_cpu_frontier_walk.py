"""The wave walk of hpmvs_amd/frontier.py (`_walk`) without a device: its two callables are served by a toy model, and the
result is compared with the obvious sequential loop over the same queue.  Integers only, no tolerance.

The toy: the "maps" are a dict cell -> int over 40 cells (start values 0 / 1); 30 leaf keys, 4 of them occupied at the start;
60 candidates per queue, each with a pre_key, a post_key, 1-5 read cells, 1-3 write cells, refined with probability 0.85, 4
images; with events on, a subtraction event of 1-3 cells precedes a candidate with probability 0.3.  A candidate's three counts
are a fixed function of the sum of the map values at its read cells and a per-candidate threshold (stages 23, 24 and 25 all
occur).  An accepted addition INCREMENTS its write cells, an event RESETS its cells to 0: additions commute with each other,
resets commute with each other, an addition and a reset do not -- the algebra of DESIGN.md section 3.9.

Every queue of the seeds below needs at least 2 waves and accepts at least 3 candidates, which is asserted: the test cannot
pass on conflict-free inputs.  Dropping any one rule of the walk (the `maybe_occ` test on pre_key, the `dirty` test on reads,
the `guard` test on writes, the `occ_guard` test on post_key, an event's `cand_guard` test, an event's cells joining `dirty`)
makes it fail."""
import random

import pytest

from hpmvs_amd.frontier import _walk

MIN = 3
N_CELLS, N_KEYS, N_CAND = 40, 30, 60
FAIL = 1    # the stage of a candidate that was not refined


def _toy(seed, with_events):
    r = random.Random(seed)
    R, W, pre, post, ref, thr, ev, queue = {}, {}, {}, {}, {}, {}, [], []
    for t in range(N_CAND):
        if with_events and r.random() < 0.3:
            queue.append(("e", len(ev)))
            ev.append({r.randrange(N_CELLS) for _ in range(r.randint(1, 3))})
        R[t] = {r.randrange(N_CELLS) for _ in range(r.randint(1, 5))}
        W[t] = {r.randrange(N_CELLS) for _ in range(r.randint(1, 3))}
        pre[t], post[t] = r.randrange(N_KEYS), r.randrange(N_KEYS)
        ref[t] = r.random() < 0.85
        queue.append(("c", t))
    occ0 = {r.randrange(N_KEYS) for _ in range(4)}
    maps0 = {c: r.randrange(2) for c in range(N_CELLS)}
    for t in range(N_CAND):
        thr[t] = r.randint(1, 4)
    return R, W, pre, post, ref, thr, ev, queue, occ0, maps0


def _run(seed, with_events):
    R, W, pre, post, ref, thr, ev, queue, occ0, maps0 = _toy(seed, with_events)
    nimg = {t: 4 for t in range(N_CAND)}

    def count(maps, t):
        s = sum(maps[c] for c in R[t])
        return (MIN if s < thr[t] else 0, MIN if s == 0 and len(R[t]) > 3 else 0, 4 if s != 1 else 2)

    def do(maps, kind, t):
        for c in (ev[t] if kind == "e" else W[t]):
            maps[c] = 0 if kind == "e" else maps[c] + 1

    # the sequential loop
    maps, occ, st, acc = dict(maps0), set(occ0), {t: FAIL for t in range(N_CAND)}, []
    for kind, t in queue:
        if kind == "e":
            do(maps, kind, t)
        elif pre[t] in occ:
            st[t] = 20
        elif ref[t]:
            v, b, f = count(maps, t)
            if not v >= MIN:
                st[t] = 23
            elif not b < MIN:
                st[t] = 24
            elif not (f >= MIN - 1 and f / nimg[t] > 0.75):
                st[t] = 25
            elif post[t] in occ:
                st[t] = 26
            else:
                occ.add(post[t]); st[t] = 0; acc.append(t); do(maps, kind, t)
    # the walk, its device behind the two callables
    maps2, occ2, st2, cnt2 = dict(maps0), set(occ0), {t: FAIL for t in range(N_CAND)}, {}
    accepted, waves, deferred = _walk(queue, pre, post, ref, nimg, R.__getitem__, W.__getitem__, ev, occ2, MIN, st2, cnt2,
                                      lambda todo: [count(maps2, t) for t in todo], lambda ops: [do(maps2, k, t) for k, t in ops])
    assert st2 == st and sorted(accepted) == acc and occ2 == occ and maps2 == maps, (seed, with_events)
    assert len(deferred) == waves and deferred[-1] == 0
    assert waves >= 2 and len(acc) >= 3, (seed, with_events, waves, len(acc))
    return waves, set(st.values())


@pytest.mark.parametrize("with_events", [False, True])
def test_walk_equals_the_sequential_loop(with_events):
    res = [_run(seed, with_events) for seed in range(500)]
    stages = set().union(*(s for _, s in res))
    assert {0, FAIL, 20, 23, 24, 25, 26} <= stages, stages
    print(f"events {with_events}: waves {min(w for w, _ in res)} .. {max(w for w, _ in res)} over {len(res)} queues")


def test_plain_frontier_round_is_one_wave():
    """sequential = False (no events): nothing is deferred, every count comes from the maps as they are at the start."""
    R, W, pre, post, ref, thr, ev, queue, occ0, maps0 = _toy(0, False)
    calls = []
    st = {t: FAIL for t in range(N_CAND)}
    accepted, waves, deferred = _walk(queue, pre, post, ref, {t: 4 for t in range(N_CAND)}, R.__getitem__, W.__getitem__, ev, set(occ0),
                                      MIN, st, {}, lambda todo: [(MIN, 0, 4)] * len(todo), calls.append, sequential=False)
    assert waves == 1 and deferred == [0] and len(calls) == 1 and [t for _, t in calls[0]] == accepted
