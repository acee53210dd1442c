"""Depth maps as jet-coloured images, the tests' side (shared by test_cpu_depth_vis.py, test_gpu_depth_vis.py and
test_gpu_cpp_visualize_depths.py): the entries of tests/golden/g9_depth_vis.npz (made by tests/golden/make_golden_depth_vis.py
with the reference's CImg), a numpy restatement of Scene::visualizeDepths' arithmetic in float32 throughout, getFullDepth
included, the host compile of hpmvs_amd/csrc/depth_vis.hpp (tests/depth_vis_host.cpp, built with g++ into a directory the
caller chooses) and the small scene whose depth maps have the golden images' shapes.

Maps are handled as api.depth_level gives them: shape (cols, rows), element [x, y] -- the transpose of the image [y, x]."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "depth_vis_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g9_depth_vis.npz")
MAX_DEPTH = np.float32(1000.0)
HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_STATE, HPMVS_ERR_NODEVICE, HPMVS_ERR_UNSUPPORTED = 0, -2, -3, -4, -5
COMBINED = -1

# the views of the GPU test's scene, 3 pyramid levels each, and their depth maps' (cols, rows) per level
VIEW_SIZES = [(70, 46), (128, 96), (11, 9), (11, 105), (5, 21)]
MAX_LEVEL = 2
MAP_SHAPES = [[(35, 23), (17, 11), (8, 5)], [(64, 48), (32, 24), (16, 12)], [(5, 4), (2, 2), (1, 1)], [(5, 52), (2, 26), (1, 13)],
              [(2, 10), (1, 5), (0, 2)]]   # (the last level of the last view is one pixel wide: a map without columns)


class Golden:
    def __init__(self):
        d = np.load(GOLDEN)
        self.lut = d["lut"]
        self.names = [str(n) for n in d["names"]]
        self.img = {n: d[n + "_in"] for n in self.names}    # float32 [H, W]
        self.rgb = {n: d[n + "_rgb"] for n in self.names}   # uint8 [H, W, 3]

    def where(self, name):
        """(view, level) of the scene's map with this image's shape"""
        h, w = self.img[name].shape
        for v, shapes in enumerate(MAP_SHAPES):
            if (w, h) in shapes:
                return v, shapes.index((w, h))
        raise KeyError(name)


# ---- the numpy restatement: float32 throughout
def colormap():
    """CImg's jet_LUT256(): four control values per channel, entry i at t_i intervals, t accumulated in float32"""
    ctl = np.array([[0, 0, 255, 255], [0, 255, 255, 0], [255, 255, 0, 0]], np.float32)
    step = np.float32(3.0) / np.float32(255.0)
    one = np.float32(1.0)
    lut = np.zeros((256, 3), np.uint8)
    t = np.float32(0.0)
    for i in range(256):
        k = int(t)
        a = np.float32(t - np.float32(k))
        for c in range(3):
            v1 = ctl[c, min(k, 3)]
            v2 = ctl[c, k + 1] if k < 3 else v1
            lut[i, c] = int(np.float32(np.float32((one - a) * v1) + np.float32(a * v2)))
        t = np.float32(t + step)
    return lut


def cell_depth(a):
    a = np.asarray(a, np.float32)
    return np.where(np.isfinite(a), a, MAX_DEPTH).astype(np.float32)


def cell_value(a):
    a = np.asarray(a, np.float32)
    return np.where(np.isfinite(a) & (a != MAX_DEPTH), a, np.float32(0.0)).astype(np.float32)


def combined(levels):
    """Scene::getFullDepth(view, 2 x, 2 y) for every cell of level 0: levels[l] of shape (cols, rows) -> (cols0, rows0)"""
    cols0, rows0 = levels[0].shape
    x, y = np.meshgrid(np.arange(cols0), np.arange(rows0), indexing="ij")
    depth = np.full((cols0, rows0), MAX_DEPTH, np.float32)
    alive = np.ones((cols0, rows0), bool)
    for l, m in enumerate(levels):
        xl, yl = x >> l, y >> l
        alive = alive & (xl < m.shape[0]) & (yl < m.shape[1])   # (the early return: nothing above counts either)
        if not alive.any():
            break
        v = np.full((cols0, rows0), MAX_DEPTH, np.float32)
        v[alive] = cell_depth(m[xl[alive], yl[alive]])
        depth = np.where(alive & (v < depth), v, depth)
    return depth


def image(map_xy, lut):
    """one map (cols, rows) -> (uint8 [rows, cols, 3], (m, M)): the empty-cell rule, normalize(0, 255), map()"""
    vals = cell_value(np.asarray(map_xy, np.float32).T)
    if vals.size == 0:
        return np.zeros(vals.shape + (3,), np.uint8), (np.float32(0.0), np.float32(0.0))
    m, M = vals.min(), vals.max()
    if m == M:
        idx = np.zeros(vals.shape, np.int64)
    elif m == 0 and M == 255:
        idx = vals.astype(np.int64)
    else:
        idx = ((vals - m) / (M - m) * np.float32(255.0) + np.float32(0.0)).astype(np.int64)
    assert idx.min() >= 0 and idx.max() <= 255
    return lut[idx], (m, M)


# ---- the host compile of depth_vis.hpp
class HostDepthVis:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libdepth_vis_host.so")
        subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        L = C.CDLL(so)
        L.dv_colormap.argtypes = [C.c_void_p]
        L.dv_level_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dv_combined.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.L = L

    def colormap(self):
        lut = np.zeros((256, 3), np.uint8)
        self.L.dv_colormap(lut.ctypes.data)
        return lut

    def image(self, map_xy):
        m = np.ascontiguousarray(map_xy, np.float32)
        cols, rows = m.shape
        rgb = np.zeros((rows, cols, 3), np.uint8)
        rng = np.zeros(2, np.float32)
        self.L.dv_level_image(m.ctypes.data, rows, cols, rgb.ctypes.data, rng.ctypes.data)
        return rgb, (rng[0], rng[1])

    def combined(self, levels):
        ms = [np.ascontiguousarray(m, np.float32) for m in levels]
        ptrs = (C.c_void_p * len(ms))(*[m.ctypes.data for m in ms])
        rows = np.array([m.shape[1] for m in ms], np.int32)
        cols = np.array([m.shape[0] for m in ms], np.int32)
        out = np.zeros(ms[0].shape, np.float32)
        self.L.dv_combined(ptrs, rows.ctypes.data, cols.ctypes.data, len(ms), out.ctypes.data)
        return out


# ---- inputs
def make_scene(sizes=VIEW_SIZES, max_level=MAX_LEVEL, seed=0xD9):
    """synth.SynthScene: the poses of synth.make_cameras, every view with its own size, random pixels (as depth_edge_inputs)"""
    from hpmvs_amd import synth
    rng = np.random.default_rng(seed)
    views = synth.make_cameras(len(sizes), 64, 48)
    for v, (w, h) in zip(views, sizes):
        v.width, v.height = w, h
        v.f = 1.2 * w
        v.rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return synth.SynthScene(views=views, covis=[[] for _ in views], max_level=max_level)


def sparse_levels(shapes, seed, fill=0.4):
    """seeded sparse maps [(cols, rows) float32] for one view: a cell holds a depth 20 .. 45 with probability `fill`"""
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        vals = rng.uniform(20.0, 45.0, size=shape).astype(np.float32)
        out.append(np.where(rng.random(size=shape) < fill, vals, MAX_DEPTH).astype(np.float32))
    return out
