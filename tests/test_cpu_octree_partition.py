"""The split into subtrees on the CPU: hpmvs_amd/csrc/octree.hpp's partition_sequential and its helpers, compiled by g++
(tests/octree_partition_host.cpp), equal the loop of the reference's getSubTrees (src/main.cpp:50-96) on the pointer tree
(tests/octree_partition_ref.py) byte for byte in every output of hpmvs_octree_partition -- on the empty tree, the 21-level chain,
a random tree of about 5 000 leaves with removed leaves and collapsed parents, and small crafted trees, the key arrays permuted,
for every min_trees and min_split_leaves of opr.MIN_TREES x opr.MIN_SPLIT_LEAVES.  The reference loop alone shows that these
inputs hold every case the order-dependent details decide.  frontier.partition's host half turns the arrays into the Octree
objects Octree.subtree gives; what the call refuses is refused with nothing written."""
import itertools

import numpy as np
import pytest

import octree_partition_ref as opr

f32 = np.float32
NAMES = list(opr.TREES)
PARAMS = list(itertools.product(opr.MIN_TREES, opr.MIN_SPLIT_LEAVES))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return opr.HostPartition(tmp_path_factory.mktemp("octree_partition_host"))


@pytest.mark.parametrize("name", NAMES + [str(n) for n in opr.EDGE_LEAVES])
def test_host_restatement_equals_the_pointer_loop(host, name):
    center, W, bk, lk = opr.tree(name)
    T = opr.pointer_tree(name)
    for min_trees, min_split in PARAMS:
        want = opr.image(T, bk, lk, min_trees, opr.loop(name, min_trees, min_split))
        rc, got = host.partition(center, W, bk, lk, min_trees, min_split)
        assert rc == 0 and not got.differences(want), (name, min_trees, min_split, got.differences(want))
        n = int(got.info[0])
        assert got.tree_leaves.sum() + got.info[1] == len(lk) == got.info[4:].sum()
        assert n <= opr.capacity(min_trees) and not got.root_key[n:].any() and not got.root_cell[n:].any()


def test_reference_loop_shows_every_case():
    shown = {}
    for name in NAMES:
        for min_trees, min_split in PARAMS:
            for case in opr.loop(name, min_trees, min_split)["shown"]:
                shown.setdefault(case, (name, min_trees, min_split))
    print("octree_partition cases:", shown)
    assert set(shown) == set(opr.CASES), set(opr.CASES) - set(shown)


def test_min_trees_below_two_is_the_root_alone(host):
    center, W, bk, lk = opr.tree("random")
    for min_trees in (-1, 0, 1):
        rc, r = host.partition(center, W, bk, lk, min_trees, 100)
        assert rc == 0 and list(r.info[:4]) == [1, 0, 0, 0] and r.root_key[0] == 1 and r.tree_leaves[0] == len(lk)
        assert not r.leaf_tree.any() and not r.branch_tree.any() and (r.leaf_sub_key == lk).all() and (r.branch_sub_key == bk).all()
        assert r.root_cell[0].tobytes() == np.array(list(center) + [W], f32).tobytes()


def _octree(name):
    from hpmvs_amd import frontier
    center, W, bk, lk = opr.tree(name)
    t = frontier.Octree(center, W, root_level=2)
    for j in np.argsort(lk):
        t.insert(int(lk[j]), ("row", int(j)))
    t.branches |= {int(k) for k in bk}                       # the branches with nothing below them
    return t


@pytest.mark.parametrize("name,min_trees,min_split", [("random", 100, 100), ("random", 65, 3), ("crafted", 9, 3), ("deep", 2, 1),
                                                      ("chain", 1, 100), ("empty", 8, 1), ("grown-700", 129, 1)])
def test_partition_host_half_equals_subtree(host, name, min_trees, min_split):
    from hpmvs_amd import api, frontier
    tree = _octree(name)
    bk = tree.branch_keys()
    lk, rows, _, _ = tree.leaf_table()
    rc, a = host.partition(tree.root_center, tree.root_width, bk, lk, min_trees, min_split)
    assert rc == 0
    P = api.OctreePartition(int(a.info[0]), int(a.info[1]), int(a.info[2]), int(a.info[3]), a.info[4:].copy(),
                            *[getattr(a, o[0]) for o in opr.OUTPUTS])
    R = frontier.partition_from_arrays(tree, bk, lk, rows, P)
    assert len(R.trees) == P.n_trees == len(R.queues) and R.stop == P.stop
    held = 0
    for t, sub in enumerate(R.trees):
        want = tree.subtree(int(R.root_key[t]))
        assert sub.branches == want.branches and sub.leaves == want.leaves and sub._below == want._below, (name, t)
        assert sub.root_center.tobytes() == want.root_center.tobytes() and sub.root_width.tobytes() == want.root_width.tobytes()
        assert sub.root_level == want.root_level == 2 + frontier.key_depth(int(R.root_key[t]))
        keys = [int(k) for k in want.leaf_table()[0]]
        assert R.queues[t] == [(want.node_level(k) * 10, k) for k in keys], (name, t)
        held += len(keys)
    assert held + len(R.orphans) == len(lk) == R.histogram.sum()
    inside = {int(k) for k in lk} - {int(k) for k in R.orphans}
    assert all(any(k >> (3 * (frontier.key_depth(k) - frontier.key_depth(int(r)))) == int(r) and k != int(r) for r in R.root_key) for k in inside)


def test_refusals_write_nothing(host):
    center, W = np.zeros(3, f32), f32(2.0)
    good_b, good_l = [0o11, 0o112], [0o1123, 0o12]
    cases = {"a leaf twice": (center, W, good_b, good_l + [0o12], 8, 100), "an orphan key": (center, W, good_b, good_l + [0o1333], 8, 100),
             "min_trees = 4097": (center, W, good_b, good_l, 4097, 100), "min_split_leaves = 0": (center, W, good_b, good_l, 8, 0),
             "a root without width": (center, f32(0.0), good_b, good_l, 8, 100),
             "a root that is not finite": (np.array([0, np.nan, 0], f32), W, good_b, good_l, 8, 100)}
    rc, ok = host.partition(center, W, good_b, good_l, 8, 100)
    assert rc == 0 and ok.info[0] == 1 and ok.root_key[0] == 0o11
    for what, (c, w, bk, lk, min_trees, min_split) in cases.items():
        rc, r = host.partition(c, w, np.array(bk, np.uint64), np.array(lk, np.uint64), min_trees, min_split, fill=0x5A)
        assert rc == -2 and all(set(b) <= {0x5A} for b in r.bytes()), what
