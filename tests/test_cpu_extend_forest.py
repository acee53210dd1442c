"""The forest form of the extend level's look-ups, host side.  The g++ build of hpmvs_amd/csrc/octree.hpp's forest code
(tests/extend_forest_host.cpp: slot ranges, the build and the check through the owning tree of every key, extend_pre / extend_post
through a tree id) equals, byte for byte, the per-tree functions (tests/extend_tree_host.cpp, which tests/test_cpu_extend_tree.py
pins to the pointer tree) run on every tree alone with its own points.  Forests: 0-6 random trees of 0-200 keys each, the keys of
a tree in random order, roots of different widths; among them trees with zero keys, a tree with one key and two trees with
identical keys under different roots.  Each kind of bad key in a middle tree: the verdict names that tree, and the lowest one when
two trees are bad."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import octree_tree_ref as otr
from test_cpu_octree_index import _random_tree

f32 = np.float32
HPMVS_ERR_ARG = -2
BAD_KEY, BAD_TWICE, BAD_ORPHAN, FOUND_OFFSETS, FOUND_PARENT, FOUND_LEVEL = 1, 2, 4, 8, 16, 32
OUT = (("skip", np.uint8), ("pre_inside", np.uint8), ("pre_key", np.uint64), ("border", np.uint8), ("post_key", np.uint64))
W0 = f32(7.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("extend_forest_host"))
    libs = []
    for name in ("extend_forest_host", "extend_tree_host"):
        so = os.path.join(d, f"lib{name}.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(otr.ROOT, "tests", name + ".cpp"),
                        "-o", so], check=True, capture_output=True)
        libs.append(C.CDLL(so))
    F, T = libs
    F.ef_slots.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    F.ef_slots.restype = None
    F.ef_tree_of.argtypes = [C.c_void_p, C.c_int, C.c_int]
    F.ef_extend.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 6
    T.et_extend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 5
    return F, T


def _poisoned(n):
    return [np.full(n, 0x5A5A if dt == np.uint64 else 0x5A, dt) for _, dt in OUT]


def _offsets(arrays):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)


def _forest(F, trees, points, point_tree, width, bf=None, lf=None):
    """trees: [(root4, bk, lk)] -> (status, outputs, found)"""
    roots = np.ascontiguousarray(np.array([t[0] for t in trees], f32).reshape(len(trees), 4))
    bf = _offsets([t[1] for t in trees]) if bf is None else np.asarray(bf, np.int32)
    lf = _offsets([t[2] for t in trees]) if lf is None else np.asarray(lf, np.int32)
    bk = np.concatenate([t[1] for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    lk = np.concatenate([t[2] for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    pt = np.ascontiguousarray(point_tree, np.int32)
    out, found = _poisoned(len(pts)), np.zeros(2, np.int32)
    rc = F.ef_extend(len(trees), roots.ctypes.data, bf.ctypes.data, lf.ctypes.data, bk.ctypes.data, lk.ctypes.data, len(pts),
                     pts.ctypes.data, pt.ctypes.data, float(width), *[a.ctypes.data for a in out], found.ctypes.data)
    return rc, out, found


def _alone(T, tree, points, width):
    root, bk, lk = tree
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    out = _poisoned(len(pts))
    rc = T.et_extend(np.ascontiguousarray(root, f32).ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, len(pts), pts.ctypes.data,
                     float(width), *[a.ctypes.data for a in out])
    return rc, out


def _tree(rng, n_leaves, scale=0):
    """A random tree of at most 200 keys under a root of width 7 * 2^scale, its keys shuffled, and points in and around it."""
    W = f32(float(W0) * 2.0 ** scale)
    if n_leaves == 0:
        center = np.array([0.5, -1.0, 2.0], f32)
        return (np.array([*center, W], f32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)), (center + rng.uniform(-0.7, 0.7, (40, 3)) * float(W)).astype(f32)
    while True:
        Tr, center, _, pts = _random_tree(rng, n_leaves, W=W)
        branches, leaves, _ = Tr.key_sets()
        if len(branches) + len(leaves) <= 200:
            break
        n_leaves = n_leaves * 2 // 3
    bk, lk = np.array(sorted(branches), np.uint64), np.array(sorted(leaves), np.uint64)
    rng.shuffle(bk)
    rng.shuffle(lk)
    around = (center + rng.uniform(-0.7, 0.7, (40, 3)) * float(W)).astype(f32)
    points = np.concatenate([pts, (pts + rng.normal(0, 0.01, pts.shape)).astype(f32), around]).reshape(-1, 3)
    return (np.array([*center, W], f32), bk, lk), points


def _random_forest(rng, n_trees):
    trees, points, owner = [], [], []
    for k in range(n_trees):
        kind = rng.integers(0, 6)
        tree, pts = _tree(rng, 0 if kind == 0 else 1 if kind == 1 else int(rng.integers(2, 45)), scale=int(rng.integers(-1, 2)))
        trees.append(tree)
        points.append(pts)
        owner += [k] * len(pts)
    points = np.concatenate(points + [np.zeros((0, 3), f32)])
    order = rng.permutation(len(points))
    return trees, points[order], np.array(owner, np.int32)[order]


def _compare(F, T, trees, points, owner, width, what):
    rc, got, found = _forest(F, trees, points, owner, width)
    assert rc == 0, (what, found)
    for k, tree in enumerate(trees):
        sel = np.nonzero(owner == k)[0]
        one, want = _alone(T, tree, points[sel], width)
        assert one == 0, (what, k)
        for (name, _), a, b in zip(OUT, got, want):
            assert a[sel].tobytes() == b.tobytes(), (what, k, name, np.nonzero(a[sel] != b)[0][:5])
    return got


def test_random_forests_equal_the_per_tree_functions(host):
    F, T = host
    rng = np.random.default_rng(11)
    sizes, skipped = [], 0
    for n_trees in (0, 1, 2, 3, 4, 5, 6, 6, 5, 3):
        trees, points, owner = _random_forest(rng, n_trees)
        for depth in (2, 4, 6):
            width = f32(float(W0) * 2.0 ** -depth)               # a level width of every root (7 / 2, 7, 14 halve onto it exactly)
            got = _compare(F, T, trees, points, owner, width, (n_trees, depth))
            skipped += int(got[0].sum())
        sizes += [len(t[1]) + len(t[2]) for t in trees]
    assert max(sizes) > 100 and max(sizes) <= 200 and skipped > 100, (sizes, skipped)
    # an explicit forest for the small trees whatever the draw: no keys, one key, no keys again
    one_key = (np.array([0.5, -1.0, 2.0, 7.0], f32), np.zeros(0, np.uint64), np.array([0o13], np.uint64))
    none = (np.array([0.0, 0.0, 0.0, 7.0], f32), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    big, pts = _tree(rng, 30)
    points = np.concatenate([pts, pts, pts, pts])
    owner = np.repeat(np.arange(4, dtype=np.int32), len(pts))
    got = _compare(F, T, [none, one_key, none, big], points, owner, f32(7.0 / 4), "small trees")
    assert got[0][owner == 0].sum() == 0 and got[0][owner == 1].sum() > 0      # nothing gates in a keyless tree; the one leaf does


def test_two_trees_with_identical_keys_do_not_meet(host):
    F, T = host
    rng = np.random.default_rng(12)
    (root, bk, lk), pts = _tree(rng, 40)
    moved = root.copy()
    moved[:3] += f32(100.0)
    fewer = lk[1:]                                                   # the same keys but one: the tables must differ in that leaf alone
    trees = [(root, bk, lk), (root, bk, lk), (moved, bk, lk), (root, bk, fewer)]
    n = len(pts)
    points = np.stack([pts, pts, pts + f32(100.0), pts], axis=1).reshape(-1, 3)      # point by point, so that the tree ids interleave
    owner = np.tile(np.arange(4, dtype=np.int32), n)
    got = _compare(F, T, trees, points, owner, f32(7.0 / 8), "identical keys")
    rows = lambda k: np.arange(k, 4 * n, 4)
    assert all(x[rows(0)].tobytes() == x[rows(1)].tobytes() for x in got)
    assert got[0][rows(0)].tobytes() != got[0][rows(3)].tobytes()    # the missing leaf gates in trees 0 and 1 only


def test_slot_ranges(host):
    F, _ = host
    counts = [(0, 0), (0, 1), (1, 0), (3, 5), (100, 100), (0, 0), (64, 64), (63, 0)]
    bf, lf = _offsets([range(b) for b, _ in counts]), _offsets([range(l) for _, l in counts])
    first = np.zeros(len(counts) + 1, np.uint64)
    F.ef_slots(len(counts), bf.ctypes.data, lf.ctypes.data, first.ctypes.data)
    size = np.diff(first.astype(np.int64))
    assert first[0] == 0
    for (b, l), s in zip(counts, size):
        assert s >= 2 and s & (s - 1) == 0 and s >= 2 * (b + l) and (s == 2 or s < 4 * (b + l)), (b, l, s)
    # the owner of every entry of a concatenated array: the tree whose range holds it, trees without keys own nothing
    for i in range(int(bf[-1])):
        k = F.ef_tree_of(bf.ctypes.data, len(counts), i)
        assert bf[k] <= i < bf[k + 1], (i, k)


def test_bad_keys_in_a_middle_tree_name_that_tree(host):
    F, T = host
    rng = np.random.default_rng(13)
    trees, points, owner = _random_forest(rng, 5)
    while min(len(t[2]) for t in trees[1:4]) < 2 or min(len(t[1]) for t in trees[1:4]) < 1:
        trees, points, owner = _random_forest(rng, 5)
    width = f32(float(W0) / 4)
    deepest = lambda lk: int(max(lk))
    kinds = {
        "zero": (lambda bk, lk: (bk, np.append(lk, np.uint64(0))), BAD_KEY),
        "the root": (lambda bk, lk: (bk, np.append(lk, np.uint64(1))), BAD_KEY),
        "off the 3-bit grid": (lambda bk, lk: (np.append(bk, np.uint64(2)), lk), BAD_KEY),
        "a branch of depth 21": (lambda bk, lk: (np.append(bk, np.uint64(1 << 63)), lk), BAD_KEY),
        "a doubled leaf": (lambda bk, lk: (bk, np.append(lk, lk[0])), BAD_TWICE),
        "a doubled branch": (lambda bk, lk: (np.append(bk, bk[0]), lk), BAD_TWICE),
        "branch and leaf": (lambda bk, lk: (np.append(bk, lk[1]), lk), BAD_TWICE),
        "an orphan": (lambda bk, lk: (bk, np.append(lk, np.uint64((deepest(lk) << 6) | 0o11))), BAD_ORPHAN),
    }
    for what, (spoil, bits) in kinds.items():
        for mid, also in ((2, None), (1, 3), (3, None)):
            bad = list(trees)
            for k in (mid, also):
                if k is not None:
                    root, bk, lk = trees[k]
                    bad[k] = (root,) + tuple(np.ascontiguousarray(a, np.uint64) for a in spoil(bk, lk))
            rc, got, found = _forest(F, bad, points, owner, width)
            assert rc == HPMVS_ERR_ARG and found[1] == mid and found[0] == bits, (what, mid, found)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _poisoned(len(points)))), what
            for k in range(5):                                       # the per-tree functions refuse that tree alone
                one, _ = _alone(T, bad[k], points[owner == k], width)
                assert (one != 0) == (k in (mid, also)), (what, k)


def test_offsets_parents_and_levels(host):
    F, _ = host
    rng = np.random.default_rng(14)
    trees, points, owner = _random_forest(rng, 4)
    width = f32(float(W0) / 4)
    bf, lf = _offsets([t[1] for t in trees]), _offsets([t[2] for t in trees])
    assert _forest(F, trees, points, owner, width)[0] == 0
    for which in ("bf", "lf"):
        off = (bf if which == "bf" else lf).copy()
        off[2] = off[1] - 1
        rc, got, found = _forest(F, trees, points, owner, width, **{which: off})
        assert rc == HPMVS_ERR_ARG and tuple(found) == (FOUND_OFFSETS, 1), (which, found)
        off = (bf if which == "bf" else lf).copy()
        off[0] = 1
        assert tuple(_forest(F, trees, points, owner, width, **{which: off})[2]) == (FOUND_OFFSETS, 0)
    for v in (-1, 4):
        pt = owner.copy()
        pt[7] = v
        pt[9] = v
        rc, got, found = _forest(F, trees, points, pt, width)
        assert rc == HPMVS_ERR_ARG and tuple(found) == (FOUND_PARENT, 7)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _poisoned(len(points))))
    # a tree whose root is as wide as the level: refused with a point, fine without one
    narrow = list(trees)
    narrow[2] = (np.array([*trees[2][0][:3], width], f32), trees[2][1], trees[2][2])
    rc, got, found = _forest(F, narrow, points, owner, width)
    assert rc == HPMVS_ERR_ARG and tuple(found) == (FOUND_LEVEL, 2)
    keep = owner != 2
    assert _forest(F, narrow, points[keep], owner[keep], width)[0] == 0
    # no tree: fine without a point, refused with one
    assert _forest(F, [], np.zeros((0, 3), f32), np.zeros(0, np.int32), width)[0] == 0
    assert _forest(F, [], np.zeros((1, 3), f32), np.zeros(1, np.int32), width)[0] == HPMVS_ERR_ARG
