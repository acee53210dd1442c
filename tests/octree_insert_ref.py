"""Test infrastructure for the batched border insertion (hpmvs_octree_insert_batch, hpmvs_octree_route_batch):
  * HostInsert: hpmvs_amd/csrc/octree.hpp's insert_sequential and a route loop over contains, compiled by g++
    (tests/octree_insert_host.cpp) into a directory the caller chooses;
  * the trees and patches the CPU and GPU tests share (the trees are built as tests/test_gpu_octree_locate.py builds its own);
  * pointer_loop: the loop of DynOctTree::addConditional on the pointer tree of tests/octree_tree_ref.py, with the class of every
    outcome read off the pointer trees alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import octree_tree_ref as otr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "octree_insert_host.cpp")
f32 = np.float32
MAX_DEPTH = 21
CLASSES = ("accepted at the static target", "accepted deeper", "static nonempty", "static too narrow", "dynamic prefix hit",
           "dynamic too narrow")


class Inserted:
    def __init__(self, n):
        self.accepted, self.leaf_key, self.blocker = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int32)

    def bytes(self):
        return [self.accepted.tobytes(), self.leaf_key.tobytes(), self.blocker.tobytes()]


class HostInsert:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "liboctree_insert_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.ot_insert.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        self.L.ot_route.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.L.ot_route.restype = None

    def insert(self, root_center, root_width, branch_key, leaf_key, points, add_width, blocker=True):
        """-> (status, Inserted)"""
        root = np.array(list(root_center[:3]) + [root_width], f32)
        bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
        lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
        pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
        n = len(pts)
        aw = np.ascontiguousarray(np.broadcast_to(np.asarray(add_width, f32), (n,)))
        r = Inserted(n)
        rc = self.L.ot_insert(root.ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, n, pts.ctypes.data, aw.ctypes.data,
                              r.accepted.ctypes.data, r.leaf_key.ctypes.data, r.blocker.ctypes.data if blocker else None)
        return rc, r

    def route(self, roots, points):
        rt = np.ascontiguousarray(roots, dtype=f32).reshape(-1, 4)
        pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
        tree = np.zeros(len(pts), np.int32)
        self.L.ot_route(len(rt), rt.ctypes.data, len(pts), pts.ctypes.data, tree.ctypes.data)
        return tree


# ---- trees: (root centre, root width, branch keys, nonempty leaf keys)

def empty_tree():
    return np.array([1, 2, 3], f32), f32(4.0), np.zeros(0, np.uint64), np.zeros(0, np.uint64)


def chain_tree():
    """branches at depths 1 .. 20 along one path, one nonempty leaf at depth 21 and one at depth 7 beside the path"""
    rng = np.random.default_rng(21)
    key, branches = 1, []
    for _ in range(20):
        key = (key << 3) | int(rng.integers(8))
        branches.append(key)
    side = (branches[5] << 3) | ((branches[6] & 7) ^ 1)
    return np.array([-0.5, 0.25, 8.0], f32), f32(3.0), np.array(branches, np.uint64), np.array([(key << 3) | 6, side], np.uint64)


@functools.lru_cache(maxsize=None)
def random_tree():
    """about 5 000 nonempty leaves at depths 3 .. 11, with removed leaves: empty leaves below branches, collapsed parents"""
    rng = np.random.default_rng(5000)
    center, W = np.array([0.5, -1.0, 2.0], f32), f32(7.0)
    T = otr.Tree(center, W)
    pts = (rng.uniform(-0.5, 0.5, (5600, 3)) * float(W) + center).astype(f32)
    for i, p in enumerate(pts):
        T.add_at(p, i, f32(float(W) * 2.0 ** -rng.uniform(3, 11)))
    for i in rng.integers(0, len(pts), 300):
        T.remove(T.at(pts[i]))
    branches, leaves, _ = T.key_sets()
    return center, W, rng.permutation(np.array(sorted(branches), np.uint64)), rng.permutation(np.array(sorted(leaves), np.uint64))


TREES = {"empty": empty_tree, "chain": chain_tree, "random": random_tree}


def key_depth(key):
    return (int(key).bit_length() - 1) // 3


def cell_of(center, W, key):
    """(c_, width_) of a path key by Cell(parent, idx)"""
    c, w = np.array(center, f32), f32(W)
    d = key_depth(key)
    for lvl in range(d):
        idx = (int(key) >> (3 * (d - 1 - lvl))) & 7
        w = f32(float(w) / 2.0)
        c = np.array([float(c[k]) + (1.0 if (idx >> k) & 1 else -1.0) * float(w) / 2.0 for k in range(3)], f32)
    return c, w


def level_widths(W):
    w = [f32(W)]
    for _ in range(MAX_DEPTH):
        w.append(f32(float(w[-1]) / 2.0))
    return w


def pointer_tree(center, W, bk, lk):
    return otr.tree_from_keys(center, W, {int(k) for k in bk}, {int(k): ("seed", j) for j, k in enumerate(lk)})


def points(rng, center, W, bk, lk, n):
    """inside, outside, on the split planes of cells of the tree (their centres), the root's faces, NaN / inf"""
    p = (center + rng.uniform(-0.5, 0.5, (n, 3)) * float(W)).astype(f32)
    kind = rng.integers(0, 10, n)
    out = kind == 0
    p[out] = (center + rng.uniform(-1.5, 1.5, (int(out.sum()), 3)) * float(W)).astype(f32)
    keys = np.concatenate([bk, lk])
    if len(keys):
        cells = {}
        for i in np.nonzero(kind == 1)[0]:
            k = int(keys[rng.integers(len(keys))])
            if k not in cells:
                cells[k] = cell_of(center, W, k)
            c, w = cells[k]
            axes = rng.random(3) < 0.6
            q = (c + rng.uniform(-0.5, 0.5, 3) * float(w)).astype(f32)
            q[axes] = c[axes]
            p[i] = q
    else:
        for i in np.nonzero(kind == 1)[0]:                    # the split planes of the root and of its children
            k = int(rng.integers(3))
            p[i, k] = f32(center[k] + float(W) * [0.0, 0.25, -0.25][int(rng.integers(3))])
    hw = f32(float(W) / 2.0)
    for i in np.nonzero(kind == 2)[0]:
        k = int(rng.integers(3))
        face = f32(center[k] + (hw if rng.random() < 0.5 else -hw))
        p[i, k] = [face, np.nextafter(face, f32(np.inf)), np.nextafter(face, f32(-np.inf))][int(rng.integers(3))]
    odd = np.nonzero(kind == 3)[0][:40]
    for j, i in enumerate(odd):
        p[i, j % 3] = [np.nan, np.inf, -np.inf][(j // 3) % 3]
    return p


def widths(rng, T0, pts, octaves=4.0):
    """log-uniform over 2 * `octaves` octaves around the width of the leaf each point falls in (T0: the pointer tree before the
    round); one in 5 is exactly the width of a level at or below that leaf -- a patch is accepted DEEPER than the target the
    unchanged tree gives it only where an earlier split left it a leaf of exactly add_width (width(d) / 2.0 > a fails at d with
    width(d) == 2 a, and the leaf found at d + 1 is not narrower than a), or for a NaN width; one in 25 is 0, negative, NaN, +inf
    or -inf"""
    n = len(pts)
    leaf_w = np.array([float(T0.at(p).w) for p in pts], np.float64)
    aw = (leaf_w * 2.0 ** rng.uniform(-octaves, octaves, n)).astype(f32)
    exact = rng.integers(0, 5, n) == 0
    aw[exact] = (leaf_w * 2.0 ** -rng.integers(0, 6, n))[exact].astype(f32)
    odd = np.nonzero(rng.integers(0, 25, n) == 0)[0]
    for j, i in enumerate(odd):
        aw[i] = [0.0, -1.0, np.nan, np.inf, -np.inf, -0.0][j % 6]
    return aw


# ---- the reference loop

def add_conditional(T, p, e, width):
    """DynOctTree::addConditional(p, width) on the pointer tree T -> (accepted, *outleaf).  otr.Tree.add_conditional does it
    wherever its splitting ends within MAX_DEPTH levels by the width; where it would not (add_width <= 0, a width below the
    deepest level's), the same steps with the product's cut at MAX_DEPTH levels (the reference goes on splitting there)."""
    width = f32(width)
    found = T.at(p)
    if not float(T.w_deepest) / 2.0 > float(width):
        leaf = T.add_conditional(p, e, width)
        return (False, found) if leaf is None else (True, leaf)
    if found.data or found.w < width:
        return False, found
    leaf = found
    while T.depth(leaf) < MAX_DEPTH and float(leaf.w) / 2.0 > float(width):
        T.split(leaf)
        leaf = T.at(p, leaf)
    leaf.data.append((p, e))
    return True, leaf


def _lowest_element(node):
    if node.children is None:
        return min((x[1] for x in node.data), default=None)
    low = [e for e in (_lowest_element(ch) for ch in node.children) if e is not None]
    return min(low, default=None)


def pointer_loop(center, W, bk, lk, pts, aw):
    """The sequential loop on the pointer tree.  -> dict(accepted [n] bool, leaf_key [n] (the leaf the patch went into or the one
    that refused it; for a static refusal the leaf of the unchanged tree), blocker [n], classes {class: count}, kind [n] (index into CLASSES), branches, leaves (the final key sets))."""
    T0 = pointer_tree(center, W, bk, lk)                       # stays as the round finds it: the static part
    T = pointer_tree(center, W, bk, lk)
    T.w_deepest = level_widths(W)[MAX_DEPTH]
    lw = level_widths(W)
    n = len(pts)
    accepted, leaf_key, blocker, kind = np.zeros(n, bool), np.zeros(n, np.uint64), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        p, a = pts[i], f32(aw[i])
        L0 = T0.at(p)
        live = T.at(p)
        ok, leaf = add_conditional(T, p, i, a)
        accepted[i], leaf_key[i] = ok, T.key(leaf)
        if L0.data or L0.w < a:                                # refused by the tree as the round finds it, and reported as
            kind[i] = 2 if L0.data else 3                      # that tree's leaf: the live one lies in it (an earlier patch may
            leaf_key[i] = T0.key(L0)                           # have split an empty L0; the reference reads no leaf of a refusal)
            k0, k1 = int(leaf_key[i]), T.key(leaf)
            assert not ok and k1 >> (3 * (key_depth(k1) - key_depth(k0))) == k0
        elif ok:
            d = T0.depth(L0)                                   # the static target: where the splitting would end from L0
            while d < MAX_DEPTH and float(lw[d]) / 2.0 > float(a):
                d += 1
            kind[i] = 0 if T.depth(leaf) == d else 1
            assert T.depth(leaf) >= d
        elif live.data:
            kind[i] = 4
            blocker[i] = live.data[0][1]
        else:
            assert live.w < a
            kind[i] = 5
            blocker[i] = _lowest_element(live.parent)          # every patch that shares the longest prefix lies below the parent
        assert ok == (kind[i] < 2) and (ok or leaf is live)
    branches, leaves, _ = T.key_sets()
    classes = {c: int((kind == k).sum()) for k, c in enumerate(CLASSES)}
    return dict(accepted=accepted, leaf_key=leaf_key, blocker=blocker, classes=classes, kind=kind, branches=branches, leaves=leaves)


def applied(bk, lk, r):
    """The key sets after the caller has entered the accepted keys of an Inserted: (branches, leaves) as sets of int."""
    branches, leaves = {int(k) for k in bk}, {int(k) for k in lk}
    for k in r.leaf_key[r.accepted != 0]:
        k = int(k)
        leaves.add(k)
        k >>= 3
        while k > 1:
            branches.add(k)
            k >>= 3
    return branches, leaves


# ---- the cases the CPU and GPU tests share: name -> (tree, points, add_width)

@functools.lru_cache(maxsize=None)
def case(name, n=3000):
    rng = np.random.default_rng(sum(name.encode()) + n)
    if name == "one-leaf":                                     # every patch in ONE empty depth-1 leaf (octant 7 of the empty tree)
        center, W, bk, lk = empty_tree()
        pts = (center + rng.uniform(0.001, 0.499, (n, 3)) * float(W)).astype(f32)
        pts[::7] = (center + (0.25 + rng.uniform(-0.01, 0.01, (len(pts[::7]), 3))) * float(W)).astype(f32)   # long shared prefixes
    else:
        center, W, bk, lk = TREES[name]()
        pts = points(rng, center, W, bk, lk, n)
        if name == "chain" and n:                              # most of the chain's volume is eight big leaves: go down the chain
            deep = int(lk[0])
            for i in range(0, n, 3):
                c, w = cell_of(center, W, deep >> (3 * int(rng.integers(0, 20))))
                pts[i] = (c + rng.uniform(-0.5, 0.5, 3) * float(w)).astype(f32)
    aw = widths(rng, pointer_tree(center, W, bk, lk), pts)
    return (center, W, bk, lk), pts, aw


def route_case(rng, n_trees, n):
    """roots [n_trees, 4], some nested in and some overlapping earlier ones, and points inside, outside and on their faces"""
    roots = np.zeros((n_trees, 4), f32)
    for t in range(n_trees):
        how = int(rng.integers(3)) if t else 0
        if how == 0:                                           # a cell of its own
            roots[t, :3], roots[t, 3] = rng.uniform(-4, 4, 3), 2.0 ** rng.integers(-2, 2)
        else:
            o = roots[int(rng.integers(t))]
            if how == 1:                                       # a child cell of an earlier root: nested, shared faces
                roots[t, 3] = f32(float(o[3]) / 2.0)
                roots[t, :3] = o[:3] + (rng.integers(0, 2, 3) * 2 - 1) * roots[t, 3] / f32(2)
            else:                                              # overlapping an earlier root
                roots[t, 3] = o[3]
                roots[t, :3] = o[:3] + rng.uniform(-0.5, 0.5, 3).astype(f32) * o[3]
    pts = rng.uniform(-6, 6, (n, 3)).astype(f32)
    if n_trees:
        for i in range(0, n, 2):                               # inside a root, and every third of those on one of its faces
            r = roots[int(rng.integers(n_trees))]
            pts[i] = r[:3] + rng.uniform(-0.5, 0.5, 3).astype(f32) * r[3]
            if i % 3 == 0:
                k = int(rng.integers(3))
                face = f32(r[k] + f32(float(r[3]) / 2.0) * (1 if rng.random() < 0.5 else -1))
                pts[i, k] = [face, np.nextafter(face, f32(np.inf)), np.nextafter(face, f32(-np.inf))][int(rng.integers(3))]
    if n > 8:
        pts[5, 0], pts[7, 2] = np.nan, np.inf
    return roots, pts
