"""A round's border queue over a forest, host side.  The g++ build of hpmvs_amd/csrc/octree.hpp's border_forest_sequential
(tests/border_forest_host.cpp: the route loop, then insert_sequential per tree over that tree's rows) equals, byte for byte, the
existing ot_route and per-tree ot_insert (tests/octree_insert_host.cpp, which tests/test_cpu_octree_insert.py pins to the pointer
tree) composed in Python.  Forests of 0 to 6 random trees of 0-200 keys under roots of different widths, and one with a keyless
tree, a one-key tree, two trees with identical key sets under different roots, two roots sharing a face and a root nested in an
earlier one; queues of about 3 000 patches whose rows interleave the trees.  The generator's outcome counts are asserted on the
host build alone: they are a condition on the inputs."""
import numpy as np
import pytest

import border_forest_ref as bfr
import octree_insert_ref as oir

f32 = np.float32
FLOOR = 50
HPMVS_ERR_ARG = -2


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("border_forest_host")
    return bfr.HostBorder(d), oir.HostInsert(d)


def _equal(hosts, trees, center, scale, what):
    B, I = hosts
    rc, got, found = B.border(trees, center, scale)
    assert rc == 0, (what, found)
    want = bfr.composed(I, trees, center, scale)
    for name, a, b in zip(("tree", "accepted", "leaf_key", "blocker"), got.bytes(), want.bytes()):
        assert a == b, (what, name, np.nonzero(getattr(got, name) != getattr(want, name))[0][:5])
    rc, none, _ = B.border(trees, center, scale, blocker=False)
    assert rc == 0 and none.bytes()[:3] == got.bytes()[:3]
    return got


def test_random_forests_equal_route_and_per_tree_insert(hosts):
    rng = np.random.default_rng(1701)
    for n_trees in (0, 1, 2, 3, 4, 5, 6):
        trees = bfr.random_forest(rng, n_trees)
        center, scale = bfr.queue(rng, trees, 600)
        got = _equal(hosts, trees, center, scale, n_trees)
        if n_trees == 0:
            assert (got.tree == -1).all() and not got.accepted.any() and not got.leaf_key.any() and (got.blocker == -1).all()
        else:
            assert len(set(got.tree.tolist()) - {-1}) == n_trees
    _equal(hosts, bfr.random_forest(rng, 3), np.zeros((0, 4), f32), np.zeros(0, f32), "no patch")


def test_special_forest_and_the_generator_outcome_counts(hosts):
    trees, center, scale = bfr.special_case()
    assert np.isnan(scale).sum() >= 5 and np.isnan(center[:, :3]).any()
    got = _equal(hosts, trees, center, scale, "special")
    kind, runs = bfr.classes(trees, center, scale, got)
    counts = {c: int((kind == k).sum()) for k, c in enumerate(bfr.CLASSES)}
    print("border_forest special", counts, "longest run", max(len(v) for v in runs.values()))
    assert min(counts.values()) >= FLOOR, counts
    assert max(len(v) for v in runs.values()) > 64
    # the same sub-key in the two trees of identical key sets, both runs with accepted members
    shared = [key for (k, key) in runs if k == 3 and (4, key) in runs and got.accepted[runs[(3, key)]].any() and got.accepted[runs[(4, key)]].any()]
    assert len(shared) >= 1
    # tree membership is interleaved: no long stretch of the queue belongs to one tree
    routed = got.tree[got.tree >= 0]
    assert (np.diff(routed) != 0).mean() > 0.5
    # the list order decides: tree 7 is a child cell of tree 0's root behind it and gets nothing; tree 8, a child cell of tree
    # 9's root ahead of it, takes that octant
    assert (got.tree == 7).sum() == 0 and (got.tree == 8).sum() >= 20 and (got.tree == 9).sum() >= 20
    # the shared face of trees 5 and 6 belongs to the lower cell alone; points on it and next to it go to both sides
    face = f32(trees[5][0][0] + f32(float(trees[5][0][3]) / 2.0))
    on = np.nonzero(center[:, 0] == face)[0]
    assert len(on) >= 3 and set(got.tree[on].tolist()) <= {5, -1} and (got.tree == 6).sum() >= 50


def test_runs_on_the_same_sub_key_of_two_trees(hosts):
    rng = np.random.default_rng(1703)
    trees = bfr.special_forest()
    center, scale = bfr.crowd(rng, trees, [(1, 150), (2, 70)])
    got = _equal(hosts, trees, center, scale, "crowd")
    _, runs = bfr.classes(trees, center, scale, got)
    assert len(runs[(1, 0o17)]) >= 150 and len(runs[(2, 0o17)]) >= 70
    assert got.accepted[runs[(1, 0o17)]].sum() >= 20 and got.accepted[runs[(2, 0o17)]].sum() >= 20
    first, last = runs[(1, 0o17)], runs[(2, 0o17)]
    assert first[0] < last[-1] and last[0] < first[-1]                       # interleaved in the queue


def test_four_root_widths_and_many_trees(hosts):
    rng = np.random.default_rng(1705)
    trees = bfr.four_widths_forest()
    assert len({float(t[0][3]) for t in trees}) == 4
    got = _equal(hosts, trees, *bfr.queue(rng, trees, 1200), "four widths")
    assert all(got.accepted[got.tree == k].sum() >= 20 for k in range(4))
    trees = bfr.many_trees_forest(130)
    got = _equal(hosts, trees, *bfr.queue(rng, trees, 1500), "130 trees")
    assert len(set(got.tree.tolist()) - {-1}) >= 120


def test_the_stand_alone_selftest_runs_clean_under_the_sanitizers(tmp_path):
    """tests/native/border_forest_selftest.cpp: the invariants on 20 000 patches over 5 trees, a program of its own built with
    AddressSanitizer and UndefinedBehaviorSanitizer (host code only; it is not loaded into Python and uses no GPU)"""
    import os
    import subprocess
    exe = str(tmp_path / "border_forest_selftest")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(bfr.ROOT, "tests", "native", "border_forest_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout, r.stderr)


def test_a_malformed_forest_names_the_lowest_tree(hosts):
    B, _ = hosts
    rng = np.random.default_rng(1706)
    trees = bfr.special_forest()
    center, scale = bfr.queue(rng, trees, 200)
    poison = bfr.Delivered(200, poison=True).bytes()
    spoil = {"no key": lambda bk, lk: (bk, np.append(lk, np.uint64(2))), "twice": lambda bk, lk: (bk, np.append(lk, lk[0])),
             "orphan": lambda bk, lk: (bk, np.append(lk, np.uint64((int(max(lk)) << 6) | 0o11)))}
    for what, fn in spoil.items():
        for bad_trees, named in (((4,), 4), ((5, 3), 3)):
            bad = list(trees)
            for k in bad_trees:
                bad[k] = (trees[k][0],) + tuple(np.ascontiguousarray(a, np.uint64) for a in fn(trees[k][1], trees[k][2]))
            rc, got, found = B.border(bad, center, scale)
            assert rc == HPMVS_ERR_ARG and found[1] == named, (what, found)
            assert got.bytes() == poison
    _, bf, lf, _, _ = bfr.flatten(trees)
    off = bf.copy()
    off[3] = off[2] - 1
    rc, got, found = B.border(trees, center, scale, bf=off)
    assert rc == HPMVS_ERR_ARG and tuple(found) == (8, 2) and got.bytes() == poison
