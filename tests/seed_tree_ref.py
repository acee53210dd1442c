"""Test infrastructure for the seed octree (hpmvs_seed_tree_batch): the host restatement (tests/seed_tree_host.cpp over
hpmvs_amd/csrc/seed_tree.hpp, built with g++ -std=c++11 -O2 -ffp-contract=off into a directory the caller chooses), the
second half of Scene::initPatches run sequentially on tests/octree_ref.py (reference Scene.cpp:183-199), and the clouds both are
compared on."""
import ctypes as C
import os
import subprocess

import numpy as np

import octree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "seed_tree_host.cpp")
f32 = np.float32
FLT_MAX, FLT_MIN = np.finfo(f32).max, np.finfo(f32).tiny
MAX_DEPTH = 21
INFO_DTYPE = np.dtype([("root_center", f32, 3), ("root_width", f32), ("scale_floor", f32), ("n_rows", np.int32),
                       ("n_leaves", np.int32)])
FIELDS = ("rows", "cell_start", "cell_center", "cell_width", "cell_level", "patch_center")


class Result:
    """The outputs of one call: info (INFO_DTYPE record), scale (floored, [n]) and the arrays of FIELDS, sized by n."""

    def __init__(self, n):
        self.info = np.zeros(1, INFO_DTYPE)
        self.scale = None
        self.rows = np.zeros(n, np.int32)
        self.cell_start = np.zeros(n + 1, np.int32)
        self.cell_center = np.zeros((n, 3), f32)
        self.cell_width = np.zeros(n, f32)
        self.cell_level = np.zeros(n, np.int32)
        self.patch_center = np.zeros((n, 3), f32)
        self.leaf_key = None

    def bytes(self):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in
                        [self.info, self.scale] + [getattr(self, k) for k in FIELDS])


class HostSeedTree:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libseed_tree_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so],
                       check=True, capture_output=True)
        L = C.CDLL(so)
        L.st_seed_tree.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.st_clamp_assoc.argtypes = [C.c_void_p] * 4
        L.st_clamp_assoc.restype = None
        L.st_depth_alone.argtypes = [C.c_float, C.c_float]
        self.L = L

    def tree(self, center, scale, ok, maxlevel):
        """-> (status, Result); center [n, 4] float32, scale [n] float32 (not modified), ok [n] uint8 or None."""
        n = len(scale)
        cen = np.ascontiguousarray(center, dtype=f32).reshape(n, 4)
        r = Result(n)
        r.scale = np.ascontiguousarray(scale, dtype=f32).copy()
        r.leaf_key = np.zeros(n, np.uint64)
        okp = None if ok is None else np.ascontiguousarray(ok, dtype=np.uint8)
        rc = self.L.st_seed_tree(n, cen.ctypes.data, r.scale.ctypes.data, None if okp is None else okp.ctypes.data, int(maxlevel),
                                 r.info.ctypes.data, r.rows.ctypes.data, r.cell_start.ctypes.data, r.cell_center.ctypes.data,
                                 r.cell_width.ctypes.data, r.cell_level.ctypes.data, r.patch_center.ctypes.data,
                                 r.leaf_key.ctypes.data)
        return rc, r

    def clamp_assoc(self, a, b, c):
        out = np.zeros(4, np.int32)
        arr = [np.ascontiguousarray(v, dtype=np.int32) for v in (a, b, c)]
        self.L.st_clamp_assoc(arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, out.ctypes.data)
        return tuple(out[:2]), tuple(out[2:])


def bounding_box(center, rows):
    """getBoundingBox (doctree.h:732-756) over center[rows], in row order: std::min / std::max, max starting at FLT_MIN."""
    if len(rows) == 0:
        return np.full(3, -1, f32), np.full(3, 1, f32)
    mn, mx = np.full(3, FLT_MAX, f32), np.full(3, FLT_MIN, f32)
    for i in rows:
        for k in range(3):
            x = center[i, k]
            if x < mn[k]:
                mn[k] = x
            if mx[k] < x:
                mx[k] = x
    return mn, mx


def sequential(center, scale, ok, maxlevel):
    """Scene.cpp:186-197 on octree_ref: -> dict(root_center, root_width, scale_floor, scale, leaves), leaves in Leaf_iterator
    order as (path key, centre, width, depth, data)."""
    center = np.ascontiguousarray(center, dtype=f32)
    scale = np.ascontiguousarray(scale, dtype=f32).copy()
    rows = [i for i in range(len(scale)) if ok is None or ok[i]]
    with np.errstate(all="ignore"):
        mn, mx = bounding_box(center, rows)
        dist = (mx - mn).astype(f32)
        inner = dist[2] if dist[1] < dist[2] else dist[1]
        width = inner if dist[0] < inner else dist[0]
        c = ((mn + mx) / f32(2.0)).astype(f32)
        floor = f32(width / f32(1 << (maxlevel + 1)))
    tree = octree_ref.OctTree(c, width, center)
    for i in rows:
        if scale[i] < floor:
            scale[i] = floor
        tree.add(i, scale[i])
    leaves = []
    for leaf in tree.nonempty():
        path, node = [], leaf
        while node is not tree.root:
            path.append(node.idx)
            node = node.parent
        path.reverse()
        key = 0
        for k, idx in enumerate(path):
            key |= idx << (3 * (MAX_DEPTH - 1 - k))
        leaves.append((key, leaf.c.copy(), f32(leaf.w), len(path), list(leaf.data)))
    return dict(root_center=c, root_width=f32(width), scale_floor=floor, scale=scale, n_rows=len(rows), leaves=leaves)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_sequential(res, center, scale, ok, maxlevel, what=""):
    """`res` (a Result, or anything with its fields) against the sequential insertion: root, floored scales, leaf paths (when res
    carries leaf_key), centres, widths, levels, leaf order and data order.  Everything bit for bit but root_center (==)."""
    ref = sequential(center, scale, ok, maxlevel)
    info = res.info[0]
    assert np.array_equal(info["root_center"], ref["root_center"]), what
    assert same_bits(info["root_width"], ref["root_width"]) and same_bits(info["scale_floor"], ref["scale_floor"]), what
    assert same_bits(res.scale, ref["scale"]), what
    L = len(ref["leaves"])
    assert int(info["n_rows"]) == ref["n_rows"] and int(info["n_leaves"]) == L, f"{what}: {info['n_leaves']} leaves, reference {L}"
    n = len(res.rows)
    data = [e for leaf in ref["leaves"] for e in leaf[4]]
    assert res.rows[:len(data)].tolist() == data and not res.rows[len(data):].any(), what
    starts = np.cumsum([0] + [len(leaf[4]) for leaf in ref["leaves"]])
    assert res.cell_start[:L + 1].tolist() == starts.tolist() and not res.cell_start[L + 1:].any(), what
    if L:
        assert same_bits(res.cell_center[:L], np.array([leaf[1] for leaf in ref["leaves"]], f32)), what
        assert same_bits(res.cell_width[:L], np.array([leaf[2] for leaf in ref["leaves"]], f32)), what
        assert res.cell_level[:L].tolist() == [leaf[3] for leaf in ref["leaves"]], what
        assert same_bits(res.patch_center[:L], np.ascontiguousarray(np.asarray(center, f32)[[leaf[4][0] for leaf in ref["leaves"]], :3])), what
        if getattr(res, "leaf_key", None) is not None:
            assert res.leaf_key[:L].tolist() == [leaf[0] for leaf in ref["leaves"]], what
    for a in (res.cell_center, res.cell_width, res.cell_level, res.patch_center):
        assert not a[L:].any(), what
    assert len(res.cell_start) == n + 1
    return ref


def _scales(rng, n, width, lo, hi):
    """scales spread over the octaves 2^lo .. 2^hi below `width`"""
    return (width * np.exp2(-rng.uniform(lo, hi, n))).astype(f32)


def clouds():
    """[(name, center [n, 4], scale [n], ok [n] or None, PATCH_INIT_MAXLEVEL)]"""
    rng = np.random.default_rng(20240611)
    out = []

    def cen(xyz):
        xyz = np.asarray(xyz, f32).reshape(-1, 3)
        return np.concatenate([xyz, np.ones((len(xyz), 1), f32)], axis=1)

    xyz = rng.uniform(-3, 5, (1500, 3))
    out.append(("random", cen(xyz), _scales(rng, 1500, 8.0, 3, 9), None, 9))
    base = rng.normal(0, 1, (60, 3))
    out.append(("coincident", cen(np.repeat(base, 10, axis=0)[rng.permutation(600)]), _scales(rng, 600, 6.0, 2, 10), None, 9))
    out.append(("all-negative", cen(-rng.uniform(1, 9, (800, 3))), _scales(rng, 800, 9.0, 2, 9), None, 9))
    # centres on split planes: the corners pin the root to [-4, 4]^3, the rest lie on multiples of 8 / 2^k
    planes = np.concatenate([[[-4, -4, -4], [4, 4, 4]], rng.integers(-32, 33, (700, 3)) / 8.0])
    out.append(("split-planes", cen(planes), _scales(rng, 702, 8.0, 1, 8), None, 9))
    out.append(("one", cen([[0.25, -1.5, 3.0]]), np.array([0.01], f32), None, 9))
    out.append(("zero", np.zeros((0, 4), f32), np.zeros(0, f32), None, 9))
    out.append(("none-ok", cen(rng.normal(0, 1, (5, 3))), np.full(5, 0.1, f32), np.zeros(5, np.uint8), 9))
    out.append(("octaves", cen(rng.normal(0, 2, (1200, 3))), _scales(rng, 1200, 12.0, 0, 14), None, 12))
    out.append(("maxlevel-0", cen(rng.uniform(0, 1, (300, 3))), _scales(rng, 300, 1.0, 0, 6), None, 0))
    out.append(("maxlevel-20", cen(rng.uniform(-1, 1, (400, 3))), _scales(rng, 400, 2.0, 4, 26), None, 20))
    xyz = rng.uniform(-2, 2, (900, 3))
    sc = _scales(rng, 900, 4.0, 2, 9)
    xyz[rng.integers(0, 900, 40), rng.integers(0, 3, 40)] = np.nan
    sc[rng.integers(0, 900, 30)] = np.nan
    sc[rng.integers(0, 900, 10)] = -1.0
    ok = (rng.uniform(0, 1, 900) < 0.8).astype(np.uint8)
    out.append(("nan-and-ok", cen(xyz), sc, ok, 9))
    return out
