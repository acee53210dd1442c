"""Test infrastructure for hpmvs_border_forest_batch, shared by the CPU and GPU tests:
  * HostBorder: hpmvs_amd/csrc/octree.hpp's border_forest_sequential compiled by g++ (tests/border_forest_host.cpp);
  * composed(): the existing ot_route and per-tree ot_insert (tests/octree_insert_host.cpp, pinned to the pointer tree by
    tests/test_cpu_octree_insert.py) composed in Python -- what the host build must equal;
  * the forests and queues: trees of tests/test_cpu_extend_forest.py's kind (0-200 keys, roots of different widths) set side by
    side, with a keyless tree, a one-key tree, two trees with identical keys under different roots, two roots that share a face and
    a root nested in an earlier one; queues whose rows interleave the trees, with widths over eight octaves around the leaf's,
    exact level widths and NaN (tests/octree_insert_ref.py: points, widths);
  * classes(): the outcome class of every row, and the runs, read off the pointer trees and the outputs."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import octree_insert_ref as oir

f32 = np.float32
ROOT = oir.ROOT
SRC = os.path.join(ROOT, "tests", "border_forest_host.cpp")
CLASSES = ("accepted", "refused by the tree", "prefix hit", "too narrow after a split", "unrouted")
W0 = f32(7.0)


class Delivered:
    def __init__(self, n, poison=False):
        self.tree = np.full(n, 0x5A5A5A5A if poison else 0, np.int32)
        self.accepted = np.full(n, 0x5A if poison else 0, np.uint8)
        self.leaf_key = np.full(n, 0x5A5A if poison else 0, np.uint64)
        self.blocker = np.full(n, 0x5A5A5A5A if poison else 0, np.int32)

    def bytes(self):
        return [self.tree.tobytes(), self.accepted.tobytes(), self.leaf_key.tobytes(), self.blocker.tobytes()]


def flatten(trees):
    """[(root4, bk, lk)] -> (roots [n, 4], branch_first, leaf_first, branch_key, leaf_key) as hpmvs_octree_forest takes them"""
    off = lambda arrays: np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)
    roots = np.ascontiguousarray(np.array([t[0] for t in trees], f32).reshape(len(trees), 4))
    bk = np.concatenate([t[1] for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    lk = np.concatenate([t[2] for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    return roots, off([t[1] for t in trees]), off([t[2] for t in trees]), bk, lk


class HostBorder:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libborder_forest_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.bf_border.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 7

    def border(self, trees, center, scale, blocker=True, bf=None, lf=None):
        """-> (status, Delivered (poisoned before the call), found [what, tree])"""
        roots, bf0, lf0, bk, lk = flatten(trees)
        bf = bf0 if bf is None else np.asarray(bf, np.int32)
        lf = lf0 if lf is None else np.asarray(lf, np.int32)
        c = np.ascontiguousarray(center, f32).reshape(-1, 4)
        s = np.ascontiguousarray(scale, f32).reshape(-1)
        r, found = Delivered(len(s), poison=True), np.zeros(2, np.int32)
        rc = self.L.bf_border(len(trees), roots.ctypes.data, bf.ctypes.data, lf.ctypes.data, bk.ctypes.data, lk.ctypes.data, len(s),
                              c.ctypes.data, s.ctypes.data, r.tree.ctypes.data, r.accepted.ctypes.data, r.leaf_key.ctypes.data,
                              r.blocker.ctypes.data if blocker else None, found.ctypes.data)
        return rc, r, found


def composed(insert_host, trees, center, scale):
    """ot_route over the roots, then ot_insert per destination tree over its rows in their given order, the blocker mapped back
    through the row selection: today's per-tree path on the host.  insert_host: an octree_insert_ref.HostInsert."""
    c = np.ascontiguousarray(center, f32).reshape(-1, 4)
    s = np.ascontiguousarray(scale, f32).reshape(-1)
    n = len(s)
    r = Delivered(n)
    r.blocker[:] = -1
    r.tree[:] = insert_host.route(np.array([t[0] for t in trees], f32).reshape(-1, 4), c[:, :3])
    aw = np.array([float(x) * 2.0 for x in s], f32)            # a double product, narrowed
    for k, (root, bk, lk) in enumerate(trees):
        sel = np.nonzero(r.tree == k)[0]
        if not len(sel):
            continue
        rc, one = insert_host.insert(root[:3], root[3], bk, lk, c[sel, :3], aw[sel])
        assert rc == 0
        r.accepted[sel], r.leaf_key[sel] = one.accepted, one.leaf_key
        r.blocker[sel] = np.where(one.blocker < 0, -1, sel[np.maximum(one.blocker, 0)])
    return r


# ---- forests: [(root4, bk, lk)]

def key_set(rng, n_leaves, scale=0):
    """the key sets of a random tree of at most 200 keys (tests/test_cpu_extend_forest.py: _tree) and its root width"""
    from test_cpu_extend_forest import _tree
    (root, bk, lk), _ = _tree(rng, n_leaves, scale=scale)
    return root[3], bk, lk


def _root(center, W):
    return np.array([*center, W], f32)


def random_forest(rng, n_trees):
    """trees side by side along x with gaps between them: keyless, one key, or random of 2 .. 44 leaves (0 .. 200 keys)"""
    trees, x = [], f32(-30.0)
    for k in range(n_trees):
        kind = int(rng.integers(0, 6))
        W, bk, lk = key_set(rng, 0 if kind == 0 else 1 if kind == 1 else int(rng.integers(2, 45)), scale=int(rng.integers(-1, 2)))
        trees.append((_root([x + rng.uniform(0, 3), rng.uniform(-2, 2), rng.uniform(-2, 2)], W), bk, lk))
        x = f32(x + 20.0)
    return trees


@functools.lru_cache(maxsize=None)
def special_forest():
    """0: random, 1: no key, 2: one key, 3 and 4: identical key sets under different roots, 5 and 6: two roots sharing a face (one
    key set each), 7: a child cell of tree 0's root AFTER it in the list (never reached), 8 before 9: a child cell of 9's root"""
    rng = np.random.default_rng(1700)
    W, bk, lk = key_set(rng, 40)
    W2, bk2, lk2 = key_set(rng, 30, scale=1)
    W3, bk3, lk3 = key_set(rng, 25, scale=-1)
    W4, bk4, lk4 = key_set(rng, 12)
    trees = [(_root([0.5, -1.0, 2.0], W), bk, lk),
             (_root([30.0, 0.0, 0.0], W0), np.zeros(0, np.uint64), np.zeros(0, np.uint64)),
             (_root([50.0, 1.0, -1.0], W0), np.zeros(0, np.uint64), np.array([0o13], np.uint64)),
             (_root([80.0, 0.0, 0.0], W2), bk2, lk2),
             (_root([180.0, 5.0, -3.0], W2), bk2, lk2),
             (_root([-40.0, 0.0, 0.0], W3), bk3, lk3),
             (_root([-40.0 + float(W3), 0.0, 0.0], W3), bk3[::-1].copy(), lk3[::-1].copy()),
             (_root([0.5 + float(W) / 4, -1.0 + float(W) / 4, 2.0 - float(W) / 4], f32(float(W) / 2)), bk4, lk4),
             (_root([-100.0 - float(W) / 4, float(W) / 4, float(W) / 4], f32(float(W) / 2)), bk4, lk4),
             (_root([-100.0, 0.0, 0.0], W), bk, lk)]
    return trees


def four_widths_forest():
    """four trees of four root widths (one wavefront each of a replay block), every one with keys of its own"""
    rng = np.random.default_rng(1704)
    trees = []
    for k, scale in enumerate((-1, 0, 1, 2)):
        W, bk, lk = key_set(rng, 20, scale=min(scale, 1))
        W = f32(float(W0) * 2.0 ** scale)
        trees.append((_root([40.0 * k, 1.0, -2.0], W), bk, lk))
    return trees


def many_trees_forest(n_trees=130):
    rng = np.random.default_rng(1730)
    sets = [key_set(rng, int(rng.integers(1, 12)), scale=int(rng.integers(-1, 2))) for _ in range(8)]
    return [(_root([20.0 * (k % 13), 20.0 * (k // 13), 0.0], sets[k % 8][0]), sets[k % 8][1], sets[k % 8][2]) for k in range(n_trees)]


def route(trees, pts):
    """the first root in list order that contains the point (Cell::contains on the pointer tree), -1"""
    T = [oir.pointer_tree(t[0][:3], t[0][3], np.zeros(0, np.uint64), np.zeros(0, np.uint64)) for t in trees]
    return np.array([next((k for k, tr in enumerate(T) if tr.contains(p)), -1) for p in pts], np.int32)


def queue(rng, trees, n, twins=(), weights={}):
    """(center [n, 4], scale [n]) of n border patches: for every row a tree drawn at random (so the trees interleave) and a point
    of octree_insert_ref.points for it -- inside, outside (into a neighbour, or into no root), on split planes, on the root's
    faces, NaN / inf --, then widths over eight octaves around the width of the leaf the row lands in, in the tree it is ROUTED
    to (octree_insert_ref.widths: one in 5 an exact level width, one in 25 zero / negative / NaN / inf).  twins: pairs (a, b) of
    trees with identical key sets: a fifth of a's points are repeated in b, moved by the difference of the roots, with the same
    scale.  weights: {tree: share of the draw} where it is not 1 (a keyless tree drawn often gets long runs in its eight leaves)."""
    center, scale = np.zeros((n, 4), f32), np.ones(n, f32)
    if n == 0 or not trees:
        center[:, :3] = rng.uniform(-50, 50, (n, 3))
        return center, scale
    share = np.array([weights.get(k, 1.0) for k in range(len(trees))])
    owner = rng.choice(len(trees), n, p=share / share.sum())
    for k, (root, bk, lk) in enumerate(trees):
        sel = np.nonzero(owner == k)[0]
        if len(sel):
            center[sel, :3] = oir.points(rng, root[:3], root[3], bk, lk, len(sel))
    dest = route(trees, center[:, :3])
    for k, (root, bk, lk) in enumerate(trees):
        sel = np.nonzero(dest == k)[0]
        if len(sel):
            aw = oir.widths(rng, oir.pointer_tree(root[:3], root[3], bk, lk), center[sel, :3])
            scale[sel] = (aw.astype(np.float64) / 2.0).astype(f32)   # (exact: the call doubles it again)
    for a, b in twins:
        rows_a, rows_b = np.nonzero(dest == a)[0], np.nonzero(owner == b)[0]
        m = min(len(rows_a), len(rows_b)) // 5 * 5
        src, dst = rows_a[:m:5], rows_b[:m:5]
        center[dst, :3] = center[src, :3] - trees[a][0][:3] + trees[b][0][:3]
        scale[dst] = scale[src]
    center[:, 3] = 1.0
    return center, scale


@functools.lru_cache(maxsize=None)
def special_case(n=3000):
    """the special forest and its queue, as the CPU and GPU tests share them (the CPU test asserts the outcome counts)"""
    trees = special_forest()
    rng = np.random.default_rng(1702 + n)
    center, scale = queue(rng, trees, n, twins=((3, 4),), weights={1: 4.0})
    root = trees[5][0]                                         # a dozen rows on the face that trees 5 and 6 share
    for i in range(10, min(n, 130), 10):
        center[i, :3] = root[:3] + rng.uniform(-0.45, 0.45, 3).astype(f32) * root[3]
        center[i, 0] = f32(root[0] + f32(float(root[3]) / 2.0))
    return trees, center, scale


def crowd(rng, trees, pairs, n_other=200):
    """runs of given sizes on the SAME sub-key of several trees, interleaved in the queue: pairs = [(tree, members)], every member
    a point of the one empty depth-1 leaf (octant 7) ... of a tree whose octant 7 is an empty leaf; n_other rows elsewhere"""
    rows = []
    for k, members in pairs:
        root = trees[k][0]
        p = (root[:3] + rng.uniform(0.001, 0.499, (members, 3)) * float(root[3])).astype(f32)
        p[::7] = (root[:3] + (0.25 + rng.uniform(-0.01, 0.01, (len(p[::7]), 3))) * float(root[3])).astype(f32)   # long shared prefixes
        s = (float(root[3]) * 2.0 ** -rng.uniform(2, 9, members) / 2.0).astype(f32)
        s[::5] = (float(root[3]) * 2.0 ** -rng.integers(2, 8, len(s[::5])) / 2.0).astype(f32)                    # exact level widths
        rows += [(p[i], s[i]) for i in range(members)]
    c2, s2 = queue(rng, trees, n_other)
    rows += [(c2[i, :3], s2[i]) for i in range(n_other)]
    order = rng.permutation(len(rows))
    center = np.ones((len(rows), 4), f32)
    center[:, :3] = np.array([rows[i][0] for i in order], f32)
    return center, np.array([rows[i][1] for i in order], f32)


def classes(trees, center, scale, r):
    """-> (kind [n] index into CLASSES, runs {(tree, static leaf key): [rows]}) for the outputs r of a delivery"""
    n = len(scale)
    kind, runs = np.zeros(n, np.int32), {}
    T0 = [oir.pointer_tree(t[0][:3], t[0][3], t[1], t[2]) for t in trees]
    for i in range(n):
        k = int(r.tree[i])
        if k < 0:
            kind[i] = 4
        elif r.accepted[i]:
            kind[i] = 0
        elif r.blocker[i] < 0:
            kind[i] = 1
        else:
            kind[i] = 2 if r.leaf_key[i] == r.leaf_key[r.blocker[i]] else 3
        if k >= 0 and kind[i] != 1:
            runs.setdefault((k, T0[k].key(T0[k].at(center[i, :3]))), []).append(i)
    return kind, runs
