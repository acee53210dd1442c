"""The batched border insertion's host restatement (tests/octree_insert_host.cpp over hpmvs_amd/csrc/octree.hpp: the static
locate, the full path, lcp against the accepted keys, insert_decide) equals the sequential loop it replaces -- a loop of
frontier.Octree.add_conditional, and of DynOctTree::addConditional on the pointer tree of tests/octree_tree_ref.py: every
decision, every key, the refusing leaf, the blocker and the final branch and leaf sets.  3 000 patches each on the empty tree,
the 21-level chain and a random tree of about 5 000 leaves, and 3 000 patches that all fall into ONE empty depth-1 leaf.  The
route loop equals Cell::contains on the pointer tree, first root in list order."""
import numpy as np
import pytest

import octree_insert_ref as oir
import octree_tree_ref as otr

f32 = np.float32
CASES = ("empty", "chain", "random", "one-leaf")
FLOOR = 50   # of every outcome class over the cases: a condition on the inputs


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return oir.HostInsert(tmp_path_factory.mktemp("octree_insert_host"))


@pytest.fixture(scope="module")
def pointer():
    """the pointer-tree loop of every case, and the classes it saw: checked before anything is compared"""
    got = {}
    for name in CASES:
        (center, W, bk, lk), pts, aw = oir.case(name)
        got[name] = oir.pointer_loop(center, W, bk, lk, pts, aw)
        print("octree_insert", name, "branches", len(bk), "leaves", len(lk), got[name]["classes"])
    total = {c: sum(got[name]["classes"][c] for name in CASES) for c in oir.CLASSES}
    assert min(total.values()) >= FLOOR, total
    assert all(got["one-leaf"]["classes"][c] >= FLOOR for c in oir.CLASSES if c.startswith("dynamic")), got["one-leaf"]["classes"]
    assert 4500 <= len(oir.random_tree()[3]) <= 5500
    return got


@pytest.mark.parametrize("name", CASES)
def test_host_restatement_equals_the_pointer_tree(host, pointer, name):
    (center, W, bk, lk), pts, aw = oir.case(name)
    ref = pointer[name]
    rc, got = host.insert(center, W, bk, lk, pts, aw)
    assert rc == 0
    bad = np.nonzero((got.accepted != 0) != ref["accepted"])[0]
    assert len(bad) == 0, (name, "decision", bad[:5], ref["kind"][bad[:5]])
    bad = np.nonzero(got.leaf_key != ref["leaf_key"])[0]
    assert len(bad) == 0, (name, "leaf key", bad[:5], ref["kind"][bad[:5]])
    bad = np.nonzero(got.blocker != ref["blocker"])[0]
    assert len(bad) == 0, (name, "blocker", bad[:5], ref["kind"][bad[:5]])
    branches, leaves = oir.applied(bk, lk, got)
    assert branches == ref["branches"] and leaves == set(ref["leaves"])
    # every accepted patch sits alone in its leaf, under its queue index
    for k, elements in ref["leaves"].items():
        for e in elements:
            if not isinstance(e, tuple):                       # (a leaf the round found nonempty holds a ("seed", j))
                assert len(elements) == 1 and int(got.leaf_key[e]) == k and got.accepted[e]
    rc, none = host.insert(center, W, bk, lk, pts, aw, blocker=False)
    assert rc == 0 and none.bytes()[:2] == got.bytes()[:2]


@pytest.mark.parametrize("name", CASES)
def test_host_restatement_equals_the_octree_loop(host, name):
    from hpmvs_amd import frontier
    (center, W, bk, lk), pts, aw = oir.case(name)
    tree = frontier.Octree(center, W)
    tree.branches = {int(k) for k in bk}
    for j, k in enumerate(lk):
        tree.leaves[int(k)] = ("seed", j)
        tree._count(int(k), +1)
    rc, got = host.insert(center, W, bk, lk, pts, aw)
    assert rc == 0
    for i in range(len(pts)):
        found = tree.at(pts[i])
        key = tree.add_conditional(pts[i], aw[i], i)
        assert (key is not None) == bool(got.accepted[i]), (name, i)
        if key is None and int(got.blocker[i]) < 0:           # refused by the tree as given: that tree's leaf, which holds `found`
            assert found >> (3 * (oir.key_depth(found) - oir.key_depth(got.leaf_key[i]))) == int(got.leaf_key[i]), (name, i)
        else:
            assert int(got.leaf_key[i]) == (found if key is None else key), (name, i)
        if key is None and int(got.blocker[i]) >= 0 and found in tree.leaves:
            assert tree.leaves[found] == int(got.blocker[i]), (name, i)
    branches, leaves = oir.applied(bk, lk, got)
    assert branches == tree.branches and leaves == set(tree.leaves)


def test_malformed_tables_are_refused(host):
    pts, aw = np.zeros((4, 3), f32), np.full(4, 0.1, f32)
    for bk, lk in (([0o11], [0o1333]), ([0o11, 0o11], []), ([], [0]), ([1], []), ([], [0o21])):
        rc, got = host.insert(np.zeros(3, f32), 2.0, np.array(bk, np.uint64), np.array(lk, np.uint64), pts, aw)
        assert rc == -2 and not got.leaf_key.any()


def test_route_takes_the_first_root_in_list_order(host):
    rng = np.random.default_rng(40)
    roots, pts = oir.route_case(rng, 40, 4000)
    got = host.route(roots, pts)
    trees = [otr.Tree(r[:3], r[3]) for r in roots]
    want = np.full(len(pts), -1, np.int32)
    later = 0                                                  # points that a later root contains as well: the order decides
    for i, p in enumerate(pts):
        inside = [t for t, T in enumerate(trees) if T.contains(p)]
        if inside:
            want[i] = inside[0]
            later += len(inside) > 1
    assert (got == want).all(), np.nonzero(got != want)[0][:5]
    assert later >= 200 and (want < 0).sum() >= 200 and len(set(want.tolist())) >= 15   # (a root nested in an earlier one never comes first)
    assert host.route(np.zeros((0, 4), f32), pts[:10]).tolist() == [-1] * 10
