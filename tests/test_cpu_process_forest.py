"""The regularize / settle sweep over a forest, host side.  The g++ build of hpmvs_amd/csrc/octree.hpp's rules
(tests/process_forest_host.cpp: the decision, the child keys, the op order and the versioned locate behind regularize) equals the
SEQUENTIAL loop of processCell on tests/octree_ref.py's pointer trees, one tree after the other: flatness bits, neighbour counts
and order, removed / split, child keys and the ordered setDepths list.  What the refinement decides -- support, which children
survive, their refined centres -- is drawn at random here, as are flatness values (NaN, 2.5, 2.6, -1 among them).  Forests of
0-6 trees, among them trees without cells, trees without keys and two trees with identical keys under different roots; the draws
are checked to hold two children in one octant, probes into removed leaves and into both empty and nonempty octants of split
leaves.  Every refusal names the lowest offender and writes nothing.  Also: frontier.process_level_forest's argument checks and
frontier.apply_sweep against the pointer tree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import octree_ref
import octree_tree_ref as otr

f32 = np.float32
HPMVS_ERR_ARG = -2
BAD_KEY, BAD_TWICE, BAD_ORPHAN, FOUND_OFFSETS, FOUND_CELL = 1, 2, 4, 8, 100
CELL_TREE, CELL_LEAF, CELL_TWICE, CELL_DEEP, CELL_REF = 0, 1, 2, 3, 4
W0 = f32(8.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("process_forest_host"))
    so = os.path.join(d, "libprocess_forest_host.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(otr.ROOT, "tests", "process_forest_host.cpp"),
                    "-o", so], check=True, capture_output=True)
    F = C.CDLL(so)
    F.pf_process.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 21
    return F


# ---- the pointer trees

def _key(tree, node):
    path = []
    while node is not tree.root:
        path.append(node.idx)
        node = node.parent
    k = 1
    for idx in reversed(path):
        k = (k << 3) | idx
    return k


def _node(tree, key):
    d = (int(key).bit_length() - 1) // 3
    n = tree.root
    for lvl in range(d):
        n = n.children[(int(key) >> (3 * (d - 1 - lvl))) & 7]
    return n


def _key_sets(tree):
    branches, leaves = [], []

    def walk(n):
        if n.children is None:
            if n.data:
                leaves.append(_key(tree, n))
            return
        if n is not tree.root:
            branches.append(_key(tree, n))
        for ch in n.children:
            walk(ch)

    walk(tree.root)
    return np.array(branches, np.uint64), np.array(leaves, np.uint64)


def _surface_tree(rng, root_center, n_points, depth):
    """A pointer tree whose leaves follow a wavy sheet through the root (so that regularize finds neighbours), cut to `depth`
    levels where it holds points; its elements are rows of tree.P (a list that grows with the sweep's children)."""
    c = np.asarray(root_center, f32)
    xy = rng.uniform(-0.5, 0.5, (n_points, 2)) * float(W0)
    z = 0.4 * np.sin(xy[:, 0]) + rng.normal(0, 0.05, n_points)
    pts = (np.column_stack([xy, z]) + c).astype(f32)
    tree = octree_ref.OctTree(c, W0, [p for p in pts])
    for e in range(n_points):
        tree.add(e, f32(float(W0) * 2.0 ** -depth * 0.9))
    return tree


class Forest:
    """trees: pointer trees.  The flat arrays are taken BEFORE the sweep; leaf order within a tree is shuffled."""

    def __init__(self, rng, trees):
        self.trees = trees
        self.roots = np.array([[*t.root.c, t.root.w] for t in trees], f32).reshape(len(trees), 4)
        bk, lk = [], []
        for t in trees:
            b, l = _key_sets(t)
            rng.shuffle(b)
            rng.shuffle(l)
            bk.append(b)
            lk.append(l)
        off = lambda a: np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.int32)
        self.bf, self.lf = off(bk), off(lk)
        self.bk = np.concatenate(bk + [np.zeros(0, np.uint64)]).astype(np.uint64)
        self.lk = np.concatenate(lk + [np.zeros(0, np.uint64)]).astype(np.uint64)
        self.lpc = np.zeros((len(self.lk), 3), f32)
        for k, t in enumerate(trees):
            for l in range(self.lf[k], self.lf[k + 1]):
                self.lpc[l] = t.P[_node(t, self.lk[l]).data[0]][:3]


def _draw_cells(rng, forest, skip_trees=()):
    """Cells: most nonempty leaves of every tree (none of skip_trees), tree by tree; everything the sweep takes as given."""
    ct, ck = [], []
    for k, t in enumerate(forest.trees):
        if k in skip_trees:
            continue
        keys = forest.lk[forest.lf[k]:forest.lf[k + 1]].copy()
        rng.shuffle(keys)
        for key in keys[:max(1, int(len(keys) * 0.8))] if len(keys) else []:
            ct.append(k)
            ck.append(key)
    n = len(ct)
    S = dict(cell_tree=np.array(ct, np.int32), cell_key=np.array(ck, np.uint64))
    S["center"] = np.zeros((n, 4), f32); S["normal"] = np.zeros((n, 4), f32); S["cam_x"] = np.zeros((n, 3), f32)
    S["flatness"] = np.zeros(n, f32); S["final"] = rng.integers(0, 2, n).astype(np.uint8); S["support"] = rng.integers(0, 4, n).astype(np.int32)
    S["child_ok"] = (rng.uniform(size=(n, 4)) < 0.6).astype(np.uint8); S["child_center"] = np.zeros((n, 4, 3), f32)
    S["ref_ok"] = np.ones(n, np.uint8)
    special = [np.nan, 2.5, 2.6, -1.0, 2.4, np.float32(2.4000001), 0.0, -0.0]
    for i in range(n):
        t = forest.trees[ct[i]]
        leaf = _node(t, ck[i])
        S["center"][i, :3] = t.P[leaf.data[0]][:3]
        S["center"][i, 3] = 1.0
        S["normal"][i, :3] = np.array([0, 0, 1], f32) + rng.normal(0, 0.15, 3).astype(f32)
        S["cam_x"][i] = np.array([1, 0, 0], f32) + rng.normal(0, 0.1, 3).astype(f32)
        r = rng.uniform()
        S["flatness"][i] = -1.0 if r < 0.4 else special[int(rng.integers(len(special)))] if r < 0.6 else rng.uniform(0, 3.0)
        for k in range(4):
            S["child_center"][i, k] = leaf.c + (rng.uniform(-0.499, 0.499, 3) * float(leaf.w)).astype(f32)
        if rng.uniform() < 0.3:
            S["child_center"][i, 1] = S["child_center"][i, 0]          # two children in one octant
            S["child_ok"][i, :2] = 1
    return S


def _reference(forest, S):
    """The sequential loop, tree after tree, on the pointer trees (which it changes)."""
    n = len(S["cell_key"])
    R = dict(flatness=S["flatness"].copy(), removed=np.zeros(n, np.uint8), split=np.zeros(n, np.uint8), children=np.zeros((n, 4), np.uint8),
             child_key=np.zeros((n, 4), np.uint64), n_neighbours=np.full(n, -2, np.int32), neighbour_key=np.zeros((n, 24), np.uint64),
             ops=[], sub=[])
    seen = dict(removed_probe=0, split_empty=0, split_child=0, same_octant=0, versioned=0)
    gone, born, cut = set(), set(), set()
    for i in range(n):
        t = forest.trees[S["cell_tree"][i]]
        leaf = _node(t, S["cell_key"][i])
        fl = S["flatness"][i]
        if fl < 0:
            f, found = octree_ref.regularize(t, S["center"][i], S["normal"][i], S["cam_x"][i], leaf.w, True, fl)
            R["flatness"][i] = f
            R["n_neighbours"][i] = len(found)
            R["neighbour_key"][i, :len(found)] = [_key(t, l) for l in found]
            for p in octree_ref.probes(S["center"][i], S["normal"][i], S["cam_x"][i], leaf.w):
                l = t.at(p)
                seen["removed_probe"] += id(l) in gone
                seen["split_child"] += id(l) in born
                seen["split_empty"] += (not l.data) and id(l.parent) in cut
            continue
        if float(fl) > 2.4:
            R["removed"][i] = 1
            R["ops"].append(i); R["sub"].append(1)
            gone.add(id(t.remove(leaf)))
            gone.add(id(leaf))
            continue
        kids = [k for k in range(4) if S["child_ok"][i, k]] if S["support"][i] >= 1 else []
        if S["support"][i] < 1 or (S["final"][i] and not kids):
            continue
        R["split"][i] = 1
        R["ops"].append(i); R["sub"].append(1)
        t.split(leaf)
        cut.add(id(leaf))
        into = []
        for k in kids:
            t.P.append(S["child_center"][i, k])
            l = t.at(S["child_center"][i, k], leaf)
            l.data.append(len(t.P) - 1)
            born.add(id(l))
            R["children"][i, k] = 1
            R["child_key"][i, k] = _key(t, l)
            into.append(_key(t, l))
            R["ops"].append(n + 4 * i + k); R["sub"].append(0)
        seen["same_octant"] += len(set(into)) < len(into)
    return R, seen


def _host(F, forest, S):
    n = len(S["cell_key"])
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    fl = S["flatness"].copy()
    out = dict(flatness=fl, removed=np.full(n, 0x5A, np.uint8), split=np.full(n, 0x5A, np.uint8), children=np.full((n, 4), 0x5A, np.uint8),
               child_key=np.full((n, 4), 0x5A5A, np.uint64), n_neighbours=np.full(n, 0x5A5A, np.int32),
               neighbour_key=np.full((n, 24), 0x5A5A, np.uint64))
    ops, sub, n_ops, found = np.full(5 * n + 1, -7, np.int32), np.full(5 * n + 1, 0x5A, np.uint8), np.full(1, -7, np.int32), np.zeros(2, np.int32)
    ins = [forest.roots, forest.bf, forest.lf, forest.bk, forest.lk, forest.lpc]
    cells = [c(S["center"], f32), c(S["normal"], f32), c(S["cam_x"], f32), c(S["ref_ok"], np.uint8), c(S["cell_tree"], np.int32),
             c(S["cell_key"], np.uint64), fl, c(S["final"], np.uint8), c(S["support"], np.int32), c(S["child_ok"], np.uint8),
             c(S["child_center"], f32)]
    outs = [out[k] for k in ("removed", "split", "children", "child_key", "n_neighbours", "neighbour_key")] + [ops, sub, n_ops, found]
    rc = F.pf_process(len(forest.trees), *[a.ctypes.data for a in ins], n, *[a.ctypes.data for a in cells], *[a.ctypes.data for a in outs])
    out["ops"], out["sub"] = (ops[:n_ops[0]].tolist(), sub[:n_ops[0]].tolist()) if rc == 0 else (None, None)
    return rc, out, tuple(found), (ops, sub, n_ops)


def _assert_equal(got, want, what):
    for k in ("flatness", "removed", "split", "children", "child_key", "n_neighbours", "neighbour_key"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.nonzero(np.atleast_1d(got[k] != want[k]))[0][:5])
    assert got["ops"] == want["ops"] and got["sub"] == want["sub"], what


def _random_forest(rng, n_trees):
    trees = []
    for k in range(n_trees):
        kind = int(rng.integers(0, 6))
        if kind == 0:      # no keys at all: eight empty leaves
            t = octree_ref.OctTree(rng.uniform(-1, 1, 3).astype(f32), W0, [])
        else:
            t = _surface_tree(rng, rng.uniform(-1, 1, 3), int(rng.integers(40, 160)), int(rng.integers(2, 4)))
        trees.append(t)
    return trees


def test_random_forests_equal_the_sequential_loop(host):
    rng = np.random.default_rng(21)
    total = dict(removed_probe=0, split_empty=0, split_child=0, same_octant=0, versioned=0)
    cells = regs = consts = rms = idle_trees = 0
    for n_trees in (0, 1, 2, 3, 4, 5, 6, 6, 4):
        trees = _random_forest(rng, n_trees)
        forest = Forest(rng, trees)
        skip = {1} if n_trees >= 3 else set()                         # a tree with keys and without cells
        S = _draw_cells(rng, forest, skip)
        rc, got, found, _ = _host(host, forest, S)
        assert rc == 0, (n_trees, found)
        idle_trees += len(skip) + sum(1 for t in trees if not _key_sets(t)[1].size)
        # regularize against the tree at the sweep's START, for the cells it can differ for
        start = {}
        for i in np.nonzero(S["flatness"] < 0)[0]:
            t = trees[S["cell_tree"][i]]
            start[i] = octree_ref.regularize(t, S["center"][i], S["normal"][i], S["cam_x"][i], _node(t, S["cell_key"][i]).w, True, S["flatness"][i])[0]
        want, seen = _reference(forest, S)
        _assert_equal(got, want, n_trees)
        for k in seen:
            total[k] += seen[k]
        total["versioned"] += sum(f32(start[i]).tobytes() != f32(want["flatness"][i]).tobytes() for i in start)
        reg = S["flatness"] < 0
        cells += len(reg); regs += int(reg.sum())
        consts += int(np.isin(want["flatness"][reg], [f32(2.5), f32(2.6)]).sum())
        rms += int((~np.isin(want["flatness"][reg], [f32(2.5), f32(2.6)])).sum())
    print(f"{cells} cells, {regs} regularized ({consts} constants, {rms} RMS values), {idle_trees} trees without cells, {total}")
    assert cells > 500 and regs > 150 and consts > 5 and rms > 50 and idle_trees >= 3
    assert all(v > 0 for v in total.values()), total


def test_two_trees_with_identical_keys_under_different_roots(host):
    rng = np.random.default_rng(22)
    a = _surface_tree(np.random.default_rng(5), np.zeros(3), 120, 3)
    shift = f32(100.0)
    # the same keys under a root moved by 100: b is built from a's points, shifted
    pts = [p + shift for p in a.P]
    b = octree_ref.OctTree(a.root.c + shift, W0, pts)
    for e in range(len(pts)):
        b.add(e, f32(float(W0) * 2.0 ** -3 * 0.9))
    assert sorted(_key_sets(a)[1].tolist()) == sorted(_key_sets(b)[1].tolist())
    forest = Forest(rng, [a, b])
    S = _draw_cells(rng, forest)
    # the same decisions for the first cells of both trees would hide a mix-up: make them differ
    S["flatness"][S["cell_tree"] == 0] = np.where(rng.uniform(size=int((S["cell_tree"] == 0).sum())) < 0.5, -1.0, 3.0).astype(f32)
    S["flatness"][S["cell_tree"] == 1] = np.where(rng.uniform(size=int((S["cell_tree"] == 1).sum())) < 0.5, -1.0, 1.0).astype(f32)
    rc, got, found, _ = _host(host, forest, S)
    assert rc == 0, found
    want, seen = _reference(forest, S)
    _assert_equal(got, want, "twins")
    assert want["removed"][S["cell_tree"] == 0].sum() > 0 and want["removed"][S["cell_tree"] == 1].sum() == 0


def test_every_refusal_names_the_lowest_offender(host):
    rng = np.random.default_rng(23)
    trees = [_surface_tree(rng, rng.uniform(-1, 1, 3), 100, 3) for _ in range(4)]
    forest = Forest(rng, trees)
    S = _draw_cells(rng, forest)
    n = len(S["cell_key"])
    assert _host(host, forest, S)[0] == 0

    def refused(S2, kind, at, forest2=forest):
        rc, got, found, (ops, sub, n_ops) = _host(host, forest2, S2)
        assert rc == HPMVS_ERR_ARG and found == (kind, at), (kind, at, rc, found)
        assert got["flatness"].tobytes() == S2["flatness"].tobytes()
        assert (got["removed"] == 0x5A).all() and (got["child_key"] == 0x5A5A).all() and (got["neighbour_key"] == 0x5A5A).all()
        assert n_ops[0] == -7 and (ops == -7).all()

    def spoil(**kw):
        S2 = {k: v.copy() for k, v in S.items()}
        for k, (at, v) in kw.items():
            S2[k][at] = v
        return S2

    lo, hi = n // 3, 2 * n // 3
    for v in (-1, 4):
        S2 = spoil(cell_tree=(hi, v))
        S2["cell_tree"][lo] = v
        refused(S2, FOUND_CELL + CELL_TREE, lo)
    for key in (0, 1, 2, int(forest.bk[forest.bf[S["cell_tree"][lo]]]), (int(S["cell_key"][lo]) << 3) | 1, 1 << 63):
        S2 = spoil(cell_key=(lo, key))
        S2["cell_key"][hi] = 0
        refused(S2, FOUND_CELL + CELL_LEAF, lo)
    # the same (tree, key) three times: the second lowest row is the offender, whichever came first
    same = np.nonzero(S["cell_tree"] == S["cell_tree"][lo])[0]
    a, b, c = same[0], same[len(same) // 2], same[-1]
    S2 = spoil(cell_key=(b, S["cell_key"][a]))
    S2["cell_key"][c] = S["cell_key"][a]
    refused(S2, FOUND_CELL + CELL_TWICE, b)
    # the same key in ANOTHER tree is no duplicate (when it is a leaf there, which the draw does not promise: look for one)
    S2 = spoil(flatness=(lo, -1.0), ref_ok=(lo, 0))
    S2["flatness"][hi] = -1.0
    S2["ref_ok"][hi] = 0
    refused(S2, FOUND_CELL + CELL_REF, lo)
    ok = spoil(flatness=(lo, 1.0), ref_ok=(lo, 0))                      # a settled cell's reference image is not looked at
    assert _host(host, forest, ok)[0] == 0
    # a cell at depth 21 that would go to branch; removed or regularized it is fine
    deep = octree_ref.OctTree(np.zeros(3, f32), W0, [np.array([0.3, 0.3, 0.3], f32)])
    deep.add(0, f32(float(W0) * 2.0 ** -21 * 0.9))
    assert (int(_key_sets(deep)[1][0]).bit_length() - 1) // 3 == 21
    f3 = Forest(rng, trees[:2] + [deep])
    S3 = _draw_cells(rng, f3)
    at = int(np.nonzero(S3["cell_tree"] == 2)[0][0])
    for fl, bad in ((1.0, True), (np.nan, True), (3.0, False), (-1.0, False)):
        S3["flatness"][at] = fl
        if bad:
            refused(S3, FOUND_CELL + CELL_DEEP, at, f3)
        else:
            assert _host(host, f3, S3)[0] == 0
    # the forest's own refusals come first and name the tree
    for which, kind in (("lk", BAD_TWICE), ("bk", BAD_KEY)):
        bad = Forest(rng, trees)
        for k in (2, 1):
            if which == "lk":
                bad.lk[bad.lf[k] + 1] = bad.lk[bad.lf[k]]
            else:
                bad.bk[bad.bf[k]] = 2
        S2 = spoil(cell_tree=(0, 9))
        rc, got, found, _ = _host(host, bad, S2)
        assert rc == HPMVS_ERR_ARG and found == (kind, 1), (which, found)
    off = Forest(rng, trees)
    off.lf = off.lf.copy()
    off.lf[2] = off.lf[1] - 1
    assert _host(host, off, S)[2] == (FOUND_OFFSETS, 1)
    # no tree: fine without a cell, refused with one
    none = Forest(rng, [])
    empty = _draw_cells(rng, none)
    assert _host(host, none, empty)[0] == 0
    one = {k: v[:1].copy() for k, v in S.items()}
    assert _host(host, none, one)[2] == (FOUND_CELL + CELL_TREE, 0)


def test_degenerate_sweeps(host):
    rng = np.random.default_rng(24)
    for what, fl in (("all regularized", -1.0), ("all settled", 1.0), ("all removed", 2.5)):
        forest = Forest(rng, [_surface_tree(np.random.default_rng(7 + k), np.zeros(3), 80, 3) for k in range(3)])
        S = _draw_cells(rng, forest)
        S["flatness"][:] = fl
        rc, got, found, _ = _host(host, forest, S)
        assert rc == 0
        want, _ = _reference(forest, S)
        _assert_equal(got, want, what)
        if fl < 0:
            assert got["ops"] == [] and not got["removed"].any() and not got["split"].any()
        if fl == 2.5:
            assert got["removed"].all() and got["sub"] == [1] * len(S["cell_key"])


# ---- frontier: argument checks and the application of a result

def test_process_level_forest_refuses_a_decreasing_cell_tree():
    from hpmvs_amd import frontier
    trees = [frontier.Octree(np.zeros(3, f32), 8.0), frontier.Octree(np.ones(3, f32), 8.0)]
    for t in trees:
        t.insert(0o13, 0)
    with pytest.raises(ValueError, match="must not decrease"):
        frontier.process_level_forest(None, _FakeBatch(2), [1, 0], [0o13, 0o13], [0.0, 0.0], trees, {}, final_level=[0, 0])
    with pytest.raises(ValueError, match="outside the list"):
        frontier.process_level_forest(None, _FakeBatch(1), [2], [0o13], [0.0], trees, {}, final_level=[0])
    with pytest.raises(ValueError, match="one entry per cell"):
        frontier.process_level_forest(None, _FakeBatch(2), [0], [0o13], [0.0], trees, {}, final_level=[0])
    with pytest.raises(ValueError, match="final_level or patch_final_minlevel"):
        frontier.process_level_forest(None, _FakeBatch(1), [0], [0o13], [0.0], trees, {})


class _FakeBatch:
    def __init__(self, n):
        self.n = n


def test_apply_sweep_equals_the_tree_operations():
    from hpmvs_amd import frontier
    rng = np.random.default_rng(25)
    P = [_surface_tree(rng, rng.uniform(-1, 1, 3), 120, 3) for _ in range(3)]
    forest = Forest(rng, P)
    S = _draw_cells(rng, forest)
    O = []
    for k, t in enumerate(P):
        o = frontier.Octree(t.root.c, t.root.w)
        for key in forest.lk[forest.lf[k]:forest.lf[k + 1]]:
            o.insert(int(key), ("seed", int(key)))
        assert o.branches == set(_key_sets(t)[0].tolist())
        O.append(o)
    want, seen = _reference(forest, S)                                   # changes the pointer trees
    frontier.apply_sweep(O, S["cell_tree"], S["cell_key"], want["removed"], want["split"], want["children"], want["child_key"])
    collapsed = 0
    for t, o in zip(P, O):
        b, l = _key_sets(t)
        assert o.branches == set(b.tolist()) and set(o.leaves) == set(l.tolist())
    n = len(S["cell_key"])
    for i in range(n):
        o = O[S["cell_tree"][i]]
        first = {}
        for k in range(4):
            if want["children"][i, k]:
                first.setdefault(int(want["child_key"][i, k]), k)
        for key, k in first.items():
            assert o.leaves[key] == ("branch", 4 * i + k)                # data[0]: the lower k of two in one octant
        if want["removed"][i]:
            collapsed += int(S["cell_key"][i]) >> 3 not in o.branches and (int(S["cell_key"][i]) >> 3) != 1
    assert want["removed"].sum() > 5 and want["split"].sum() > 5 and seen["same_octant"] > 0
    print(f"{int(want['removed'].sum())} removed ({collapsed} parents collapsed), {int(want['split'].sum())} split")
    # rows given: the first child's row
    o = frontier.Octree(np.zeros(3, f32), 8.0)
    o.insert(0o13, "old")
    frontier.apply_sweep([o], [0], [0o13], [0], [1], [[1, 1, 0, 1]], [[0o135, 0o135, 0, 0o131]], rows=["a", "b", "c", "d"])
    assert o.leaves == {0o135: "a", 0o131: "d"} and o.branches == {0o13}
