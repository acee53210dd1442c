"""Inputs for the depth-map entry points at the edges of their rules (needs no GPU; shared by test_cpu_depth_edge_inputs.py and
test_gpu_depth_edges.py).  None of those entry points reads a pixel, so the views hold random bytes and nothing is rendered.

Scene A: 70 views (a second, partly filled chunk of 64 lanes) of six different sizes, odd and even, 6 pyramid levels: the
         levels run down to 1 pixel, whose depth map has 0 rows.
Scene B: 5 views of two sizes, 8 pyramid levels (HPMVS_MAX_LEVELS).
Patches: 1 500 per scene, lists of up to 256 ids (repeats allowed), inside the frustums, on their borders, outside, behind a
         camera; scales whose rounded level runs from below 0 to above the last level.  No NaN / inf and no id outside the
         scene (the oracle would index out of bounds).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_DEPTH = np.float32(1000.0)
MAX_IMAGES = 256
N_PATCHES = 1500
SIZES = {"A": [(45, 37), (64, 48), (37, 45), (91, 61), (33, 33), (128, 35)], "B": [(141, 131), (200, 129)]}
N_VIEWS = {"A": 70, "B": 5}
MAX_LEVEL = {"A": 5, "B": 7}
SEED = {"A": 0xD0A, "B": 0xD0B}
LIST_LENGTHS = np.array([0, 1, 2, 3, 5, 8, 63, 64, 65, 130, 256])
LIST_SHARE = np.array([0.04, 0.10, 0.15, 0.19, 0.16, 0.12, 0.05, 0.05, 0.05, 0.05, 0.04])


def make_scene(which: str):
    """synth.SynthScene: the poses of synth.make_cameras, every view with its own size, f = 1.2 * width, random pixels."""
    from hpmvs_amd import synth
    rng = np.random.default_rng(SEED[which])
    views = synth.make_cameras(N_VIEWS[which], 64, 48)
    sizes = SIZES[which]
    for i, v in enumerate(views):
        v.width, v.height = sizes[i % len(sizes)]
        v.f = 1.2 * v.width
        v.rgb = rng.integers(0, 256, size=(v.height, v.width, 3), dtype=np.uint8)
    return synth.SynthScene(views=views, covis=[[] for _ in views], max_level=MAX_LEVEL[which])


@dataclass
class Patches:
    center: np.ndarray    # [n, 4] float32, w = 1
    normal: np.ndarray    # [n, 4] float32, w = 0
    scale: np.ndarray     # [n] float32
    n_images: np.ndarray  # [n] int32
    images: np.ndarray    # [n, MAX_IMAGES] int32, unused slots -1

    @property
    def n(self):
        return len(self.scale)

    def take(self, idx):
        idx = np.asarray(idx)
        return Patches(self.center[idx].copy(), self.normal[idx].copy(), self.scale[idx].copy(), self.n_images[idx].copy(),
                       self.images[idx].copy())

    def batch(self):
        from hpmvs_amd import api
        return api.Batch(self.center, self.normal, self.scale, self.n_images, self.images)

    def oracle(self):
        """orc.Patch[n] (filled through the struct's own offsets, not field by field)."""
        from oracle import oracle as orc
        arr = (orc.Patch * self.n)()
        v = orc.patch_view(arr)
        v["center"][:] = self.center; v["normal"][:] = self.normal; v["scale"][:] = self.scale
        v["n_images"][:] = self.n_images; v["images"][:, :self.images.shape[1]] = self.images
        return arr


def make_patches(scene, which: str, n: int = N_PATCHES) -> Patches:
    rng = np.random.default_rng(SEED[which] + 1)
    V = scene.n_views
    kind = rng.random(n)                       # 60 % inside most frustums, 30 % borders and outside, 10 % behind a camera
    half = np.where(kind < 0.6, 9.0, 16.0)
    c = np.empty((n, 3))
    c[:, :2] = rng.uniform(-1.0, 1.0, size=(n, 2)) * half[:, None]
    c[:, 2] = rng.uniform(-1.0, 1.0, size=n)
    behind = kind >= 0.9
    behind_view = rng.integers(0, V, size=n)
    u = rng.uniform(1.05, 1.5, size=n)
    cams = np.stack([v.c for v in scene.views])
    c[behind] = cams[behind_view[behind]] * u[behind, None]
    g = rng.normal(size=(n, 3))
    g[:, 2] = np.abs(g[:, 2]) + 1e-3
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    scale = 2.0 ** rng.uniform(-6.0, 3.0, size=n)
    n_images = rng.choice(LIST_LENGTHS, size=n, p=LIST_SHARE).astype(np.int32)
    images = np.full((n, MAX_IMAGES), -1, np.int32)
    for k in range(n):
        m = int(n_images[k])
        images[k, :m] = rng.integers(0, V, size=m)
        # the camera a patch lies behind is in its list (short lists over 70 views would hardly ever name it, and only an
        # attached view takes a negative depth as far as depthTest and setDepths: viewBlockTest drops it at the projection)
        if behind[k] and m > 0:
            images[k, rng.integers(0, m)] = behind_view[k]
    center = np.concatenate([c, np.ones((n, 1))], axis=1).astype(np.float32)
    normal = np.concatenate([g, np.zeros((n, 1))], axis=1).astype(np.float32)
    return Patches(center, normal, scale.astype(np.float32), n_images, images)


def camera_depths(oscene, P: Patches) -> np.ndarray:
    """[n, V] float32: the depth of every patch in every view, the third row of the oracle's camera matrix applied in its
    own order (every pyramid level has the same third row)."""
    rows = np.array([list(oscene.camera(v).P[0])[8:12] for v in range(oscene.n_views)], dtype=np.float32)
    x = P.center
    return ((rows[None, :, 0] * x[:, None, 0] + rows[None, :, 1] * x[:, None, 1]) + rows[None, :, 2] * x[:, None, 2]) \
        + rows[None, :, 3] * x[:, None, 3]


def attached_depths(oscene, P: Patches) -> np.ndarray:
    """[n, MAX_IMAGES] float32: the depth in attached image k (NaN for the unused slots)."""
    z = camera_depths(oscene, P)
    ids = np.where(P.images >= 0, P.images, 0)
    out = np.take_along_axis(z, ids, axis=1)
    out[np.arange(MAX_IMAGES)[None, :] >= P.n_images[:, None]] = np.nan
    return out


def setters(oscene, P: Patches) -> np.ndarray:
    """[n] bool: the depth is positive in every attached view.  The reference CHECK-fails on a negative depth, the oracle
    would write it, the device skips it (a documented departure), so only these patches enter maps that are compared."""
    z = attached_depths(oscene, P)
    return ~(z <= 0).any(axis=1)   # (NaN: unused slot)


def map_shapes(oscene, n_levels: int):
    """{(view, level): (cols, rows)} -- the shape of OracleDepths.level / api.depth_level arrays, element [x, y]."""
    from oracle import oracle as orc
    D = orc.OracleDepths(oscene)
    return {(v, l): D.level(v, l).shape for v in range(oscene.n_views) for l in range(n_levels)}


def random_fill(shapes, seed: int):
    """{(view, level): float32 map}: every cell 1000 with probability 0.5, else uniform in [20, 45] (the depths of the scene)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in sorted(shapes):
        shape = shapes[key]
        vals = rng.uniform(20.0, 45.0, size=shape).astype(np.float32)
        out[key] = np.where(rng.random(size=shape) < 0.5, MAX_DEPTH, vals).astype(np.float32)
    return out


def fill_oracle(D, maps):
    for (v, l), m in maps.items():
        D.level(v, l)[...] = m


def fill_gpu(gpu, maps):
    from hpmvs_amd import api
    for (v, l), m in maps.items():
        if m.size == 0:
            continue   # (a 0-row level: nothing to copy)
        m = np.ascontiguousarray(m, dtype=np.float32)
        api._chk(api.lib().hpmvs_scene_depth_set_level(gpu.h, v, l, m.ctypes.data, m.shape[1], m.shape[0]))


def oracle_maps(D, shapes):
    return {key: D.level(*key).copy() for key in shapes}


def gates(D, P_oracle, idx, margin=1.0, abs_int=0) -> np.ndarray:
    """[len(idx), 3] int32: n_visible, n_blocking, n_free of the oracle."""
    return np.array([D.gates(P_oracle[int(k)], margin, abs_int) for k in idx], dtype=np.int32).reshape(len(idx), 3)


def map_views(D, shapes):
    """{(view, level): the oracle's own map, writable, no copy} -- valid while D lives."""
    return {key: D.level(*key) for key in shapes if shapes[key][0] * shapes[key][1]}


def written_cells(views):
    """The set of (view, level, x, y) whose cell is below 1000 (views: map_views)."""
    out = set()
    for (v, l), m in views.items():
        xs, ys = np.nonzero(m < MAX_DEPTH)
        out.update((v, l, int(x), int(y)) for x, y in zip(xs, ys))
    return out


def n_written(D, shapes) -> int:
    views = D if isinstance(D, dict) else map_views(D, shapes)
    return sum(int((m < MAX_DEPTH).sum()) for m in views.values())


def block_cells(shapes, sizes0, n_levels, view, ix0, iy0):
    """The cells Scene::getFullDepth can read for 3x3 level-0 pixel blocks: arrays view, ix0, iy0 (top-left pixels) ->
    [m, 4] rows (view, level, x, y).  Of each block the pixels inside the image, each at (px // 2 >> l, py // 2 >> l) for
    l = 0, 1, ... up to the first level where that cell is out of range."""
    view = np.asarray(view, dtype=np.int64)
    if view.size == 0:
        return np.zeros((0, 4), np.int64)
    dx, dy = np.meshgrid(np.arange(3), np.arange(3))
    px = (np.asarray(ix0, dtype=np.int64)[:, None] + dx.reshape(1, 9)).ravel()
    py = (np.asarray(iy0, dtype=np.int64)[:, None] + dy.reshape(1, 9)).ravel()
    vv = np.repeat(view, 9)
    w0 = np.array([s[0] for s in sizes0], dtype=np.int64)[vv]
    h0 = np.array([s[1] for s in sizes0], dtype=np.int64)[vv]
    alive = (px >= 0) & (px < w0) & (py >= 0) & (py < h0)
    cols = np.array([[shapes[(v, l)][0] for l in range(n_levels)] for v in range(len(sizes0))], dtype=np.int64)
    rows = np.array([[shapes[(v, l)][1] for l in range(n_levels)] for v in range(len(sizes0))], dtype=np.int64)
    out = []
    for l in range(n_levels):
        x, y = (px // 2) >> l, (py // 2) >> l
        alive = alive & (x < cols[vv, l]) & (y < rows[vv, l])
        if not alive.any():
            break
        out.append(np.stack([vv[alive], np.full(int(alive.sum()), l, np.int64), x[alive], y[alive]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def read_cells(shapes, sizes0, n_levels, frees_p, attached_p, view_block_p, with_view_block=True, with_frees=True):
    """The cells the footprints of ONE patch name as read: the `frees` cells, and the blocks of its `attached` rows and of
    its `view_block` rows with flag 1.  [m, 4] rows (view, level, x, y)."""
    parts = []
    if with_frees:
        parts.append(frees_p[frees_p[:, 0] >= 0].astype(np.int64))
    a = attached_p[attached_p[:, 0] >= 0]
    parts.append(block_cells(shapes, sizes0, n_levels, a[:, 0], a[:, 1], a[:, 2]))
    if with_view_block:
        seen = np.nonzero(view_block_p[:, 0] == 1)[0]
        parts.append(block_cells(shapes, sizes0, n_levels, seen, view_block_p[seen, 1], view_block_p[seen, 2]))
    return np.concatenate(parts)


class MixedMaps:
    """Oracle maps that hold fill 2 everywhere except at chosen cells, which hold fill 1."""

    def __init__(self, D, shapes, fill1, fill2):
        self.D, self.shapes, self.f1, self.f2 = D, shapes, fill1, fill2
        fill_oracle(D, fill2)
        self.views = map_views(D, shapes)

    def counts_with(self, cells, patch, margin=1.0, abs_int=0):
        """The oracle's counts of `patch` with `cells` ([m, 4]: view, level, x, y) from fill 1; fill 2 is restored after."""
        touched = []
        if len(cells):
            key = cells[:, 0] * 16 + cells[:, 1]
            order = np.argsort(key, kind="stable")
            cells, key = cells[order], key[order]
            starts = np.nonzero(np.diff(key, prepend=-1))[0].tolist() + [len(key)]
            for a, b in zip(starts[:-1], starts[1:]):
                v, l = int(cells[a, 0]), int(cells[a, 1])
                x, y = cells[a:b, 2], cells[a:b, 3]
                self.views[(v, l)][x, y] = self.f1[(v, l)][x, y]
                touched.append((v, l, x, y))
        got = self.D.gates(patch, margin, abs_int)
        for v, l, x, y in touched:
            self.views[(v, l)][x, y] = self.f2[(v, l)][x, y]
        return got
