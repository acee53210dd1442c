"""hpmvs_amd/csrc/level_walk.hpp without a device: the rule "an item's outcome from its earlier neighbours only, by rounds" --
the one the kernels of hpmvs_level_walk_batch are compiled from -- built by g++ (tests/level_walk_host.cpp) and driven through two
callbacks, as frontier._walk is, must give what frontier._walk gives: stages, counts, the accepted candidates in their order,
waves, deferrals per wave, occupancy and maps.  Integers only, no tolerance.

The queues are those of tests/test_cpu_frontier_walk.py widened with two to four key sets, border candidates, candidates without a
pre key and leaves taken at the start (tests/level_walk_ref.py).  What makes them hard is asserted on the host walk alone: every
queue needs at least 2 waves, and over the seeds an event is deferred and the stages 26 and 27 occur."""
import os
import subprocess

import pytest

import level_walk_ref as lw
from level_walk_ref import BORDER, EVENT, FAIL, HAS_PRE, MIN, POST_TAKEN, PRE_TAKEN, REFINED


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return lw.HostWalk(tmp_path_factory.mktemp("level_walk_host"))


SHAPES = [(60, 40, 10), (120, 200, 10), (80, 12, 6)]   # (candidates, cells, keys per set): the last is the dense one


@pytest.mark.parametrize("with_events", [False, True])
def test_rounds_equal_the_walk(host, with_events):
    stages, late_event, waves, most_rounds = set(), False, [], 0
    for seed in range(240):
        T = lw.Toy(seed, with_events, *SHAPES[seed % 3])
        want, late = lw.run_walk(T)
        assert want[3] >= 2, (seed, want[3])                  # (the host walk: no queue is conflict-free)
        got, rounds = lw.run_rounds(host, T)
        for k, name in enumerate(("stage", "counts", "accepted", "waves", "deferred per wave", "occupancy", "maps")):
            assert got[k] == want[k], (seed, with_events, name)
        assert len(rounds) == want[3] and min(rounds) >= 1
        stages |= set(want[0].values()); late_event |= late; waves.append(want[3]); most_rounds = max(most_rounds, max(rounds))
    assert {0, FAIL, 20, 23, 24, 25, 26, 27} <= stages, stages
    assert late_event == with_events                          # (some queue defers an event)
    print(f"events {with_events}: waves {min(waves)} .. {max(waves)}, at most {most_rounds} rounds in a wave")


def _hand(host, items, flow, anti, gate=(MIN, 0, 4)):
    """items: (flags, set, pre, post) per queue item; flow / anti: lists per NODE.  Every gate pass gives `gate`."""
    flags, sets, pre, post = zip(*items)
    stage = [0 if f & EVENT else FAIL for f in flags]
    applied = []
    rc, st, counts, acc, wave, n_waves, rounds = host.walk(flags, sets, pre, post, lw.csr(flow) + lw.csr(anti), [4] * len(items), stage,
                                                           lambda todo: [gate] * len(todo), lambda ops, ev: applied.append((ops, ev)))
    assert rc == 0
    return st.tolist(), counts.tolist(), acc.tolist(), wave.tolist(), n_waves, rounds, applied


C = REFINED | HAS_PRE


def test_event_after_a_writer_and_before_a_reader(host):
    """c0 writes cell X, e writes X, c1 reads X.  The event waits for c0's addition (wave 2), c1 for the event (wave 3).  c1 needs no
    round of its own: an event before it in its flow list defers it whatever the event becomes."""
    items = [(C, 0, 1, 11), (EVENT, 0, 0, 0), (C, 0, 2, 12)]
    flow, anti = [[], [0], [0, 1]], [[], [], []]
    st, counts, acc, wave, n_waves, rounds, applied = _hand(host, items, flow, anti)
    assert (st, acc, wave, n_waves) == ([0, 0, 0], [1, 0, 1], [1, 2, 3], 3)
    assert applied == [([0], False), ([1], True), ([2], False)] and rounds == [2, 1, 1]


def test_event_before_a_reader_and_a_writer(host):
    """e writes X, c0 reads X, c1 writes X.  The event applies at once; c0's counts must see it (wave 2); c1 may not overwrite what
    the deferred c0 reads, and gives its counts back (wave 2, after c0)."""
    items = [(EVENT, 0, 0, 0), (C, 0, 1, 11), (C, 0, 2, 12)]
    flow, anti = [[], [0], []], [[], [], [0, 1]]
    st, counts, acc, wave, n_waves, rounds, applied = _hand(host, items, flow, anti)
    assert (st, acc, wave, n_waves) == ([0, 0, 0], [0, 1, 1], [1, 2, 2], 2)
    assert applied == [([0], True), ([1, 2], False)] and counts[2] == [MIN, 0, 4]


def test_a_chain_of_five_candidates_on_one_leaf_key(host):
    """Five candidates whose refined patches share a leaf: the first takes it, each of the others is a stage 26 -- in ONE wave and
    two rounds: all wait for the first, and once it holds the leaf none needs to know what the ones between become."""
    items = [(C, 0, 100 + k, 7) for k in range(5)]
    st, counts, acc, wave, n_waves, rounds, applied = _hand(host, items, [[]] * 5, [[]] * 5)
    assert (st, acc, wave, n_waves, rounds) == ([0, 26, 26, 26, 26], [1, 0, 0, 0, 0], [1] * 5, 1, [2])
    assert applied == [([0], False)] and all(c == [MIN, 0, 4] for c in counts)


def test_a_deferred_unrefined_candidate_guards_its_pre_key(host):
    """e writes what c0 reads, so c0 (post key 7) is deferred; c1, NOT refined, sits in leaf 7 before refinement: it may be gated
    by c0 later, so it is deferred too and guards key 7; c2's refined patch goes to leaf 7: deferred, counts given back.  Wave 2
    accepts c0, and with leaf 7 taken c1 is a stage 20 and c2 a stage 26."""
    items = [(EVENT, 0, 0, 0), (C, 0, 1, 7), (HAS_PRE, 0, 7, 0), (C, 0, 3, 7)]
    flow, anti = [[], [0], []], [[], [], []]          # nodes: e, c0, c2
    st, counts, acc, wave, n_waves, rounds, applied = _hand(host, items, flow, anti)
    assert (st, acc, wave, n_waves) == ([0, 0, 20, 26], [0, 1, 0, 0], [1, 2, 2, 2], 2)
    assert counts[2] == [-1, -1, -1] and counts[3] == [MIN, 0, 4] and rounds == [3, 2]
    # with c0 failing its counts in wave 2 the leaf stays free: c1 keeps its preset stage, c2 is accepted
    calls = []
    flags, sets, pre, post = zip(*items)
    rc, st, counts, acc, wave, n_waves, rounds = host.walk(
        flags, sets, pre, post, lw.csr(flow) + lw.csr(anti), [4] * 4, [0, FAIL, FAIL, FAIL],
        lambda todo: calls.append(todo) or [(0, 0, 4) if i == 1 else (MIN, 0, 4) for i in todo], lambda ops, ev: None)
    assert (rc, st.tolist(), acc.tolist(), wave.tolist()) == (0, [0, 23, FAIL, 0], [0, 0, 0, 1], [1, 2, 2, 2]) and calls == [[1, 3], [1, 3]]


def test_taken_leaves_and_flag_bytes_that_cannot_occur(host):
    items = [(C | PRE_TAKEN, 0, 1, 2), (C | POST_TAKEN, 0, 3, 4), (REFINED | BORDER, 0, 0, 0), (REFINED, 0, 1, 5), (0, 0, 0, 0)]
    st, counts, acc, wave, n_waves, rounds, applied = _hand(host, items, [[]] * 4, [[]] * 4)
    assert (st, acc, wave, rounds) == ([20, 26, 27, 0, FAIL], [0, 0, 0, 1, 0], [1] * 5, [1])
    assert counts == [[-1] * 3, [MIN, 0, 4], [MIN, 0, 4], [MIN, 0, 4], [-1] * 3]
    for bad in (EVENT | REFINED, EVENT | BORDER, 64, 128):
        rc = host.walk([bad], [0], [0], [0], lw.csr([[]]) + lw.csr([[]]), [4], [0], lambda t: [], lambda o, e: None)[0]
        assert rc == -1, bad
    assert host.walk([], None, [], [], lw.csr([]) + lw.csr([]), [], [], lambda t: [], lambda o, e: None)[5] == 0   # n == 0: no wave


def test_the_stand_alone_selftest_runs_clean_under_the_sanitizers(tmp_path):
    """tests/native/level_walk_selftest.cpp: walk_by_rounds against an in-program sequential loop, a program of its own built
    with AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "level_walk_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(lw.ROOT, "tests", "native", "level_walk_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
