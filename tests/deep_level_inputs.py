"""Inputs for the photometric kernels on pyramid levels 5 and 6 and on views of several sizes in one scene (needs no GPU;
shared by test_cpu_deep_level_inputs.py and test_gpu_deep_levels.py).

Scene D: 8 views (the poses of synth.make_cameras) whose sizes cycle through 1283x1031, 1536x1152, 1021x1279, 1400x1050 --
         odd and even widths and heights, a level-6 image of 20x16 pixels -- f = 1.2 * width, 8 pyramid levels
         (HPMVS_MAX_LEVELS), every view covisible with every other.  Each view is rendered by synth's numpy renderer at 1/8
         size and repeated 8 x 8 (a second instead of a minute): from level 3 on the blocks are gone, and the numpy renderer
         gives the same bytes on every machine.
Seeds:   600 per START_LEVEL 5 and 6 (synth.make_seeds works per view size), over synth's square of +-8 world units.  A
         level-6 image is 20x16 pixels or less and the texture's shortest wave is hardly more than one of its pixels, so
         nearly every level-6 seed of that square fails before the optimiser; a third set, "6c", seeds level 6 within +-1.5
         units of the scene centre, where the windows fit, and reaches the optimiser a few dozen times.
Options: the defaults with MAXLEVEL = 7 (sampleTexture then reaches level 6, addImages level 4) and MIN_IMAGES_PER_PATCH = 2.
Sweeps:  24 walks of a patch across one side of sampleTexture's bounding-box gate (PatchOptimizer.cpp:503-508): levels 0, 5
         and 6, a view of even and one of odd width, four sides; 289 positions 1/288 level pixel apart along the view's image
         axis, from half a pixel inside the limit to half a pixel outside (1/288: float32 centres and projections move a
         level-0 position by up to ~1e-4 pixel, and neighbours are to stay within 1/256 of each other as the oracle sees
         them).  The limit is located with a float64 model of the gate (below); what the reference's float32 arithmetic
         decides at each position is for the oracle to say.  16 finer walks on levels 5 and 6 stand on the limit itself.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

SIZES = [(1283, 1031), (1536, 1152), (1021, 1279), (1400, 1050)]
N_VIEWS = 8
MAX_LEVEL = 7                  # 8 pyramid levels
N_SEEDS = 600
SEED_SETS = {"5": (5, 8.0), "6": (6, 8.0), "6c": (6, 1.5)}   # name -> (START_LEVEL, extent of the seeded square around the origin)
SHRINK = 8
SIDES = ("left", "top", "right", "bottom")
SWEEP_LEVELS = (0, 5, 6)
SWEEP_VIEWS = {0: (3, 2), 5: (1, 2), 6: (3, 0)}   # level -> (a view of even width, a view of odd width)
SWEEP_STEPS = 289              # 1/288 level pixel apart: one pixel in all
WINDOW_ZOOM = 2.0 ** -0.25     # a sweep patch's sample step in level pixels (its level is round(log2) of this times 2^level)
FINE_STEPS = 193               # the fine walks: 2^-21 level pixel apart, +-4.6e-5 pixel around the model's limit
FINE_STEP = 2.0 ** -21
MAX_IMAGES = 32


def make_scene():
    """synth.SynthScene D."""
    from hpmvs_amd import synth
    views = synth.make_cameras(N_VIEWS, 64, 48)
    tex = synth.make_texture(24, lambda_min=1.7)
    for i, v in enumerate(views):
        W, H = SIZES[i % len(SIZES)]
        v.width, v.height, v.f = W, H, 1.2 * W
        small = synth.View(-(-W // SHRINK), -(-H // SHRINK), v.f / SHRINK, v.q, v.c)
        img = synth._render_numpy(small, tex)
        v.rgb = np.ascontiguousarray(np.repeat(np.repeat(img, SHRINK, axis=0), SHRINK, axis=1)[:H, :W])
    covis = [[b for b in range(N_VIEWS) if b != a] for a in range(N_VIEWS)]
    return synth.SynthScene(views=views, covis=covis, max_level=MAX_LEVEL, texture=tex)


def make_seeds(scene, which: str):
    """`which` in SEED_SETS."""
    from hpmvs_amd import synth
    level, extent = SEED_SETS[which]
    return synth.make_seeds(scene, N_SEEDS, start_level=level, max_images=MAX_IMAGES, max_seed_images=8, seed=synth.SEED + level,
                            displace=0.3, extent=extent)


def set_options(o):
    """`o`: api.default_options() or orc.default_options() (the same fields)."""
    o.MAXLEVEL = 7
    o.MIN_IMAGES_PER_PATCH = 2
    return o


def gpu_options():
    from hpmvs_amd import api
    return set_options(api.default_options())


def oracle_options():
    from oracle import oracle as orc
    return set_options(orc.default_options())


def odd_width(scene, view: int) -> bool:
    return scene.views[view].width % 2 == 1


# ---- a float64 model of sampleTexture's geometry: good to ~1e-5 pixel, enough to put a sweep around the limit ----------
def _pose(view):
    from hpmvs_amd import synth
    return synth._R_from_quat(view.q), np.asarray(view.c, dtype=np.float64)


def _project(view, X, level):
    R, c = _pose(view)
    pc = R @ (X - c)
    return np.array([(view.f * pc[0] / pc[2] + view.width / 2.0), (view.f * pc[1] / pc[2] + view.height / 2.0)]) / (1 << level)


def model_level(view, X, scale, max_level=MAX_LEVEL - 1):
    """Camera::getLeveli."""
    _, c = _pose(view)
    r = scale * (2.0 * view.f) / (2.0 * np.linalg.norm(X - c))
    return int(min(max(round(math.log2(r)), 0), max_level))


def model_margins(scene, X, normal, scale, ref_view, view):
    """(level, [left, top, right, bottom]): how far inside each side of the gate the window's bounding box lies in `view`, in
    level pixels (negative: outside), for the patch axes calculatePatchAxis forms from `ref_view`."""
    Rr, _ = _pose(scene.views[ref_view])
    unit = lambda a: a / np.linalg.norm(a)
    z = unit(normal)
    y = unit(np.cross(z, Rr[0]))
    x = unit(np.cross(y, z)) * scale
    y = y * scale * float(np.dot(y, Rr[1]))
    v = scene.views[view]
    lvl = model_level(v, X, scale)
    pc = _project(v, X, lvl)
    dx, dy = _project(v, X + x, lvl) - pc, _project(v, X + y, lvl) - pc
    corners = np.array([pc + sx * 3.5 * dx + sy * 3.5 * dy for sx in (-1, 1) for sy in (-1, 1)])
    mn, mx = corners.min(axis=0), corners.max(axis=0)
    W, H = v.width >> lvl, v.height >> lvl
    return lvl, np.array([mn[0] - 3.0, mn[1] - 3.0, (W - 3) - mx[0], (H - 3) - mx[1]])


def _angle_ok(scene, X, normal, view, cos_max=math.cos(math.radians(55.0))):
    _, c = _pose(scene.views[view])
    d = c - X
    return float(np.dot(d / np.linalg.norm(d), normal / np.linalg.norm(normal))) > cos_max


@dataclass
class Sweep:
    level: int
    view: int       # the view whose gate is walked
    side: str       # "left" / "top" / "right" / "bottom"
    slot: int       # the slot of `view` in every patch's list (slot 0 is the reference image of setINCCs(0))
    first: int      # its patches are first .. first + count - 1 of the batch, from inside to outside
    count: int = SWEEP_STEPS

    @property
    def rows(self):
        return slice(self.first, self.first + self.count)


def _point(view, a, b, level, depth):
    """The world point `depth` in front of the camera that projects to level-`level` pixel (a, b)."""
    R, c = _pose(view)
    s = float(1 << level)
    return c + depth * (R.T @ np.array([(a * s - view.width / 2.0) / view.f, (b * s - view.height / 2.0) / view.f, 1.0]))


def _one_sweep(scene, level, view, side, ref, offsets):
    """Positions of one sweep, `offsets` level pixels outwards of where the model has the limit, with the patch axes of view
    `ref`, or None where the model does not find the other three sides (and, for ref != view, the whole gate of `ref`) passed
    with room to spare at both ends."""
    v = scene.views[view]
    k = SIDES.index(side)
    W, H = v.width >> level, v.height >> level
    depth = 30.0
    mid = np.array([W / 2.0, H / 2.0])
    axis = k % 2                                   # 0: walk along x, 1: along y
    X0 = _point(v, mid[0], mid[1], level, depth)
    _, c = _pose(v)
    scale = WINDOW_ZOOM * (1 << level) * np.linalg.norm(X0 - c) / v.f
    normal = (c - X0) / np.linalg.norm(c - X0)

    def at(t):
        p = mid.copy()
        p[axis] = t
        return _point(v, p[0], p[1], level, depth)

    def margin(t):
        lvl, m = model_margins(scene, at(t), normal, scale, ref, view)
        return m[k] if lvl == level else float("nan")

    lo, hi = (0.0, mid[axis]) if k < 2 else (mid[axis], float((W, H)[axis]))   # the margin changes sign between the two
    inside, outside = (hi, lo) if k < 2 else (lo, hi)
    if not (margin(inside) > 0 > margin(outside)):
        return None
    for _ in range(60):
        t = 0.5 * (inside + outside)
        if margin(t) > 0:
            inside = t
        else:
            outside = t
    sign = -1.0 if k < 2 else 1.0                  # towards the outside
    ts = inside + sign * offsets
    for t in (ts[0], ts[-1]):
        X = at(t)
        lvl, m = model_margins(scene, X, normal, scale, ref, view)
        if lvl != level or np.delete(m, k).min() < 0.25:
            return None
        if ref != view:
            _, mr = model_margins(scene, X, normal, scale, ref, ref)
            if mr.min() < 1.0 or not _angle_ok(scene, X, normal, ref):
                return None
    return np.array([at(t) for t in ts]), normal, scale


def make_sweeps(scene, fine: bool = False):
    """(synth.Seeds of 24 * 289 patches -- fine: 16 * 193 --, [Sweep]).  Every patch has two images: the walked view and a neighbour.  Where the
    model finds a neighbour whose own window passes along the whole walk, the neighbour is the reference image and the walked
    view sits in slot 1 (setINCCs gives 2.0 for that slot alone when its gate fails); otherwise the walked view is the
    reference in slot 0 (every entry is 2.0 when it fails, entry 0 is 0.0 when it passes) and the second image is one that sees
    the patch, if any does: no other view reaches the top and the bottom of the one portrait size.

    fine: the same walks on levels 5 and 6 only, 193 positions 2^-21 level pixel apart around the limit.  A float32 centre
    moves the box by about that much per unit in its last place there, about as much as one of the box's own, so most walks
    put the box's edge on the limit itself (tests/test_cpu_deep_level_inputs.py counts which): the one position that tells
    `<` from `<=`.  (On level 0 a centre's last place is worth 200 of the box's, and no walk would find it.)"""
    from hpmvs_amd import synth
    sweeps, C, N, S, I = [], [], [], [], []
    count = FINE_STEPS if fine else SWEEP_STEPS
    offsets = (np.arange(count) - count // 2) * (FINE_STEP if fine else 1.0 / (SWEEP_STEPS - 1.0))
    for level in (SWEEP_LEVELS[1:] if fine else SWEEP_LEVELS):
        for view in SWEEP_VIEWS[level]:
            for side in SIDES:
                got, slot, other = None, 0, (view + 1) % N_VIEWS
                neighbours = [(view + d) % N_VIEWS for d in (1, N_VIEWS - 1, 2, N_VIEWS - 2, 3, N_VIEWS - 3, 4)]
                for u in neighbours:
                    got = _one_sweep(scene, level, view, side, u, offsets)
                    if got is not None:
                        slot, other = 1, u
                        break
                if got is None:
                    got = _one_sweep(scene, level, view, side, view, offsets)
                    assert got is not None, (level, view, side)
                    X, normal, scale = got
                    for u in neighbours:   # a second image whose window passes at both ends, if there is one: windows get compared
                        if all(model_margins(scene, x, normal, scale, view, u)[1].min() > 0.3 and _angle_ok(scene, x, normal, u)
                               for x in (X[0], X[-1])):
                            other = u
                            break
                X, normal, scale = got
                sweeps.append(Sweep(level, view, side, slot, count * len(sweeps), count))
                C.append(np.concatenate([X, np.ones((len(X), 1))], axis=1))
                N.append(np.tile(np.concatenate([normal, [0.0]]), (len(X), 1)))
                S.append(np.full(len(X), scale))
                I.append(np.tile([other, view] if slot == 1 else [view, other], (len(X), 1)))
    n = count * len(sweeps)
    images = np.full((n, MAX_IMAGES), -1, np.int32)
    images[:, :2] = np.concatenate(I)
    seeds = synth.Seeds(center=np.concatenate(C).astype(np.float32), normal=np.concatenate(N).astype(np.float32),
                        scale=np.concatenate(S).astype(np.float32), n_images=np.full(n, 2, np.int32), images=images,
                        truth=np.zeros((n, 3)))
    return seeds, sweeps


def describe(sweep: Sweep) -> str:
    return f"level {sweep.level} view {sweep.view} {sweep.side} side, slot {sweep.slot}, patches {sweep.first}..{sweep.first + sweep.count - 1}"


# ---- what the oracle alone says about these inputs ----------------------------------------------------------------------
def grabs(osc, P, options, ref_slot=0):
    """[(patch, slot, view, ok, level)] of sampleTexture for every attached image of every oracle patch, axes from `ref_slot`."""
    from oracle import oracle as orc
    out = []
    for k in range(len(P)):
        for j in range(P[k].n_images):
            ok, _, lvl, _ = orc.sample_texture(osc, P[k], ref_slot, j, options)
            out.append((k, j, int(P[k].images[j]), bool(ok), lvl if ok else -1))
    return out


def window_edge(osc, patch, sweep: Sweep, options):
    """(the float32 coordinate of the bounding box's edge on the sweep's side, the window's centre / dx / dy) as sampleTexture
    computes them, also where the gate fails (orc.sample_texture reports its geometry only where it passes): the same call with MAXLEVEL = the
    sweep's level clamps to the level above, where every coordinate is exactly twice as large and the gate is passed with room.
    Levels 5 and 6 only."""
    from oracle import oracle as orc
    f32 = np.float32
    o = orc.Options.from_buffer_copy(options)
    o.MAXLEVEL = sweep.level
    ok, _, lvl, geo = orc.sample_texture(osc, patch, 0, sweep.slot, o)
    assert ok and lvl == sweep.level - 1
    geo = (geo * f32(0.5)).astype(f32)
    c, dx, dy, h = geo[0:2], geo[2:4], geo[4:6], f32(3.5)
    corners = np.array([(c - h * dx) - h * dy, (c + h * dx) - h * dy, (c - h * dx) + h * dy, (c + h * dx) + h * dy], dtype=f32)
    k = SIDES.index(sweep.side)
    edge = corners[:, k % 2].min() if k < 2 else corners[:, k % 2].max()
    return edge, geo


def objective_grabs(osc, patch, x, options) -> int:
    """The sampleTexture calls of objective_fn at x that pass their gates: 0 where the reference image fails (objective_fn
    returns before it looks at the others), else 1 + the others that pass.  Read off the oracle's own objective: over the list
    [ref, a] with MIN_IMAGES_PER_PATCH = 2 it is 2.0 exactly when one of the two grabs fails (a robust incc is at most 2/7),
    and the frame at x depends on the patch and its first image only."""
    from oracle import oracle as orc
    o = orc.Options.from_buffer_copy(options)
    o.MIN_IMAGES_PER_PATCH = 2
    ids = list(patch.images[:patch.n_images])
    q = orc.Patch()
    q.center[:] = patch.center[:]; q.normal[:] = patch.normal[:]; q.scale = patch.scale
    q.n_images = 2
    q.images[0] = ids[0]
    passed = []
    for a in ids:
        q.images[1] = a
        passed.append(orc.objective_at(osc, q, x, o) != 2.0)
    return int(sum(passed)) if passed[0] else 0
