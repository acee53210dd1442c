"""Inputs that reach the late rejection stages of refinement on small scenes: the cases of tests/test_cpu_stage_inputs.py
(the oracle alone reaches what is claimed here) and tests/test_gpu_stage_parity.py (the device against the oracle on them).
No GPU in this file: scenes are rendered with numpy, so the device and the oracle get the very arrays the counts below were
measured on.

A case names its scene, how its patches are made, the option overrides, and for each stage the minimum number of patches the
ORACLE must leave there (`minimum`).  The minimums are conditions on the generator, about half of what was measured (never
more than the coverage asked for needs), so that a change to hpmvs_amd/synth.py that moves a histogram fails on the CPU.

Stages (oracle/hpmvs_oracle.c, orc_optimize / orc_init_patches / orc_expand): 0 refined; 1 addImages; 2 filterImagesNCC(alpha 1);
3 assureImageAngles before the optimiser; 4 optimizePatch; 5 addImages again; 6 filterImagesNCC(alpha 2); 7 filterImagesByAngle;
8 assureImageAngles after the optimiser; 9 filterImagesNCC behind setRefImage; 10 too few measurements; 11 fewer than two
measurements inside their image; 12 drifted; 20 candidate not built / skipped / outside its leaf; 22 refined candidate too far.

Measured with the oracle and the genuine NLopt (`python tests/stage_inputs.py` prints this table; `nlopt` is the histogram of
nlopt_result over the patches with nevals > 0, `acos` the number of patches whose result changes when the oracle's acos() is
correctly rounded -- the one class of patch the device may differ in, so a case must not hold more than one):

    refine case          stages                                          nlopt                  acos
    min_angle_40         0: 135, 2: 6, 3: 51, 8: 8                       1: 142, 4: 1           0
    min_angle_40_long    0: 126, 2: 5, 3: 59, 8: 10                      1: 136                 0
    min_angle_25_v3      0: 160, 2: 13, 3: 27                            1: 158, 4: 2           0
    set_ref_image        0: 45, 1: 293, 2: 6, 6: 48, 9: 8                1: 101                 0
    gate_edge            0: 352, 1: 1, 2: 43, 6: 2, 7: 1, 9: 1           1: 351, 4: 5           0
    behind_the_plane     0: 151, 1: 1, 2: 92, 3: 65, 4: 91               1: 147, 4: 4           0
    roundoff             0: 396, 2: 3, 4: 1                              1: 388, 4: 8, -4: 1    0

    seed-loop case       stages                                                                 acos
    seed_min_angle_40    0: 209, 1: 2, 2: 15, 3: 60, 8: 20, 10: 40, 11: 20, 12: 34              0

    expansion case       stages                                                                 acos
    extend_min_angle_40  0: 179, 2: 52, 3: 41, 8: 20, 20: 64, 22: 28                            0
    branch_min_angle_40  0: 111, 2: 36, 3: 48, 8: 24, 20: 8, 22: 29                             0

(The same seeds as `roundoff` at START_LEVEL 2 hold the -4 patch too, and beside it one patch of the acos class; START_LEVEL 1
holds none.)

How the late stages are reached.  MIN_ANGLE 40 deg on the 12-view ring (neighbours 18 deg apart) leaves few pairs of attached
views far enough apart: the list fails assureImageAngles before the optimiser (3), or after it once filterImagesNCC(alpha 2) and
filterImagesByAngle have thinned it (8).  MIN_IMAGES_PER_PATCH 5 with NCC_ALPHA_2 0.8 at START_LEVEL 1 makes the last
filterImagesNCC, behind setRefImage's new reference image, fall below the minimum (9).  Stage 7 and stage 4 were believed
unreachable; a search of 1 200 oracle runs (480 000 patches: 3 and 12 views, START_LEVEL 1-2, both list lengths, normals tilted by
0-100 deg, MAX_ANGLE 20-120 deg, MIN_IMAGES_PER_PATCH 2 / 3 / 5) found both:
  * 7 (gate_edge): sampleTexture gates an image by `cos < cos((double)MAX_ANGLE)`, filterImagesByAngle keeps it by
    `cos > cosf(MAX_ANGLE)`.  An image passes the first and fails the second only when its float cosine EQUALS cosf(MAX_ANGLE) and
    cosf rounded up -- one float, but the objective jumps to 2.0 behind the gate, so BOBYQA walks minima onto that very edge.
    4 patches of the 480 000; 35 deg is a MAX_ANGLE whose cosf rounds up.
  * 4 by image count (behind_the_plane): with MAX_ANGLE beyond 90 deg an attached view behind the patch plane survives
    filterImagesNCC, sortImages drops it (cos <= 0) and optimizePatch finds fewer than MIN_IMAGES_PER_PATCH.  Below 90 deg every
    survivor of stage 2 has a positive cosine, so the count cannot fall there.
  * 4 by result code (roundoff): NLopt returns -4 (ROUNDOFF_LIMITED) for one patch in a few hundred thousand; 7 in the search.
    MAXEVAL (5) never occurred.
5 (addImages only appends) and 21 (the candidate's scale is 0.9 width / 2 by construction) stay unreachable by valid input.
"""
import collections

import numpy as np

SCENES = {"v12": dict(n_views=12, width=640, height=480, n_waves=24),
          "v3": dict(n_views=3, width=640, height=480, n_waves=24)}
OPTION_FIELDS = ("MAXLEVEL", "MINLEVEL", "MAX_ANGLE", "MIN_ANGLE", "MAX_IMAGES_PER_PATCH", "MIN_IMAGES_PER_PATCH",
                 "NCC_ALPHA_1", "NCC_ALPHA_2")

Case = collections.namedtuple("Case", "name scene args options minimum results", defaults=({},))


def rad(deg):
    """An angle option as tests/test_gpu_random_scenes.py writes it: the float32 nearest to the radians."""
    return float(np.float32(np.deg2rad(deg)))


MIN_ANGLE_40 = dict(MIN_ANGLE=rad(40))

_scenes = {}


def scene(name):
    """The named scene, rendered once per process with numpy."""
    from hpmvs_amd import synth
    if name not in _scenes:
        _scenes[name] = synth.make_scene(**SCENES[name])
    return _scenes[name]


def save_scenes(path):
    """Every scene, rendered, into one file: a child process loads them instead of rendering again."""
    import pickle
    with open(path, "wb") as fh:
        pickle.dump({name: scene(name) for name in SCENES}, fh)


def load_scenes(path):
    import pickle
    with open(path, "rb") as fh:
        _scenes.update(pickle.load(fh))


def apply_options(o, overrides):
    """Set a case's overrides on an options struct (the oracle's or the library's: same field names)."""
    for k, v in overrides.items():
        assert k in OPTION_FIELDS, k
        setattr(o, k, v)
    return o


def tilt_normals(seeds, deg, seed=5):
    """The seeds with every normal turned by `deg` about a random axis perpendicular to it: seeds that arrive with attached
    views near or behind their plane."""
    from hpmvs_amd import synth
    rng = np.random.default_rng(seed)
    n = seeds.normal[:, :3].astype(np.float64)
    a = rng.normal(size=n.shape)
    a -= (a * n).sum(axis=1, keepdims=True) * n
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    t = np.deg2rad(deg)
    out = seeds.normal.copy()
    out[:, :3] = (n * np.cos(t) + a * np.sin(t)).astype(np.float32)
    out[:, :3] /= np.sqrt((out[:, :3] ** 2).sum(axis=1, dtype=np.float32))[:, None]
    return synth.Seeds(center=seeds.center, normal=out, scale=seeds.scale, n_images=seeds.n_images, images=seeds.images,
                       truth=seeds.truth)


# ---- refine: api.optimize_batch against orc.optimize_batch

def refine_cases():
    def seeds(n, start_level, m, d, tilt=0):
        return dict(n=n, start_level=start_level, max_seed_images=m, displace=d, tilt=tilt)
    return [
        Case("min_angle_40", "v12", seeds(200, 2, 3, 0.5), MIN_ANGLE_40, {0: 60, 2: 3, 3: 25, 8: 5}),
        Case("min_angle_40_long", "v12", seeds(200, 2, 8, 1.5), MIN_ANGLE_40, {0: 60, 3: 25, 8: 5}),
        Case("min_angle_25_v3", "v3", seeds(200, 2, 3, 0.5), dict(MIN_ANGLE=rad(25)), {0: 80, 2: 6, 3: 13}),
        Case("set_ref_image", "v12", seeds(400, 1, 3, 0.5), dict(MIN_IMAGES_PER_PATCH=5, NCC_ALPHA_2=0.8, MAX_ANGLE=rad(40)),
             {0: 20, 1: 150, 6: 24, 9: 5}),
        Case("gate_edge", "v3", seeds(400, 2, 3, 0.5), dict(MAX_ANGLE=rad(35)), {0: 170, 2: 20, 7: 1}),
        Case("behind_the_plane", "v3", seeds(400, 2, 8, 1.5, tilt=80), dict(MAX_ANGLE=rad(120)), {0: 75, 2: 45, 3: 30, 4: 45}),
        Case("roundoff", "v3", seeds(400, 1, 3, 0.5, tilt=60), dict(MAX_ANGLE=rad(89), MIN_IMAGES_PER_PATCH=2), {0: 190, 4: 1},
             results={-4: 1}),
    ]


# What the case set as a whole has to reach, in the oracle: {stage: patches in at least one case}.
REFINE_REQUIRED = {1: 5, 2: 5, 3: 5, 6: 5, 8: 5, 9: 5,      # each beside >= 20 successes in some case
                   4: 1, 7: 1}                              # what the search found beyond what was asked for
NLOPT_RESULTS_REQUIRED = {1, 4, -4}                         # codes that occur somewhere in the refine cases
SEED_LOOP_REQUIRED = {0: 5, 3: 5, 8: 5, 10: 5, 11: 5, 12: 5}
EXPAND_REQUIRED = {0: 3, 2: 3, 3: 3, 8: 3, 20: 3, 22: 3}    # per mode


def refine_seeds(case):
    from hpmvs_amd import synth
    a = case.args
    s = synth.make_seeds(scene(case.scene), a["n"], start_level=a["start_level"], max_images=32,
                         max_seed_images=a["max_seed_images"], displace=a["displace"])
    return tilt_normals(s, a["tilt"]) if a["tilt"] else s


# ---- seed loop: api.init_patches_batch against orc.init_patches

def seed_loop_cases():
    return [Case("seed_min_angle_40", "v12", dict(n=400, start_level=2, noise=0.5), MIN_ANGLE_40,
                 {0: 100, 3: 30, 8: 10, 10: 20, 11: 10, 12: 15})]


def seed_loop_points(case):
    """(xyz, meas_off, meas_img, start_level): synth's NVM points with every 8th moved 6-40 units sideways out of the views'
    frusta, its measurement list kept (stage 11, or on with the measurements that still see it), and every 10th list cut to two
    measurements (stage 10)."""
    from hpmvs_amd import synth
    a = case.args
    n = a["n"]
    xyz, off, img = synth.make_nvm_points(scene(case.scene), n, start_level=a["start_level"], noise=a["noise"])
    xyz = xyz.copy()
    rng = np.random.default_rng(11)
    moved = np.arange(3, n, 8)
    ang, r = rng.uniform(0, 2 * np.pi, len(moved)), rng.uniform(6, 40, len(moved))
    xyz[moved, 0] += r * np.cos(ang)
    xyz[moved, 1] += r * np.sin(ang)
    lists = [img[off[i]:off[i + 1]] for i in range(n)]
    for i in range(5, n, 10):
        lists[i] = lists[i][:2]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return xyz, off, np.concatenate(lists).astype(np.int32), a["start_level"]


# ---- expansion: api.expand_batch against orc.expand_batch

def expand_cases():
    return [Case("extend_min_angle_40", "v12", dict(mode=0, n_parents=64, width_factor=0.6), MIN_ANGLE_40,
                 {0: 90, 2: 25, 3: 20, 8: 10, 20: 30, 22: 14}),
            Case("branch_min_angle_40", "v12", dict(mode=1, n_parents=64, width_factor=1.2), MIN_ANGLE_40,
                 {0: 55, 2: 18, 3: 24, 8: 12, 20: 4, 22: 14})]


def expand_inputs(case, oracle_scene):
    """(mode, parents as an orc.Patch array, cell_center, cell_width, skip).  The parents are patches the ORACLE refined under the
    default options; of them, in order, those with a candidate the oracle ends at 3 or 8 under the case's options and then the
    others, n_parents in all (so that few parents hold what is looked for).  Leaves as tests/test_gpu_expand.py makes them,
    narrower (width_factor) so that refined candidates leave them (22)."""
    from hpmvs_amd import synth
    from oracle import oracle as orc
    a = case.args
    mode, N = a["mode"], (6 if a["mode"] == 0 else 4)
    seeds = synth.make_seeds(scene(case.scene), 400, start_level=2, max_images=32, max_seed_images=3, displace=0.5)
    P = orc.patches_from_seeds(seeds)
    orc.optimize_batch(oracle_scene, P, n_threads=8)
    refined = [k for k in range(len(P)) if P[k].stage == 0]

    def geometry(par):
        pv = orc.patch_view(par)
        rng = np.random.default_rng(3 + mode)
        width = (pv["scale"] * (2.0 / 0.9) * a["width_factor"]).astype(np.float32)
        cc = (pv["center"][:, :3] + rng.uniform(-0.3, 0.3, (len(par), 3)).astype(np.float32) * width[:, None]).astype(np.float32)
        skip = (rng.uniform(size=len(par) * N) < 0.15).astype(np.uint8) if mode == 0 else None
        return cc, width, skip

    def pick(idx):
        par = (orc.Patch * len(idx))()
        for j, k in enumerate(idx):
            par[j] = P[k]
        return par

    everyone = pick(refined)
    out = orc.expand_batch(oracle_scene, mode, everyone, *geometry(everyone),
                           options=apply_options(orc.default_options(), case.options), n_threads=8)
    st = np.array([q.stage for q in out]).reshape(len(refined), N)
    late = ((st == 3) | (st == 8)).any(axis=1)
    order = [k for k, h in zip(refined, late) if h][:a["n_parents"] // 2]
    order += [k for k in refined if k not in order][:a["n_parents"] - len(order)]
    par = pick(sorted(order))
    return (mode, par) + geometry(par)


# the oracle's fields the device is compared in (x is not: its acos-born last bits are tests/test_gpu_optimize.py's subject)
COMPARED = ("stage", "nlopt_result", "nevals", "fmin", "center", "normal", "scale", "color", "n_images", "images")


def histogram(values):
    return dict(sorted(collections.Counter(int(v) for v in values).items()))


def result_histogram(patches):
    """nlopt_result over the patches whose optimiser ran."""
    return histogram(p.nlopt_result for p in patches if p.nevals > 0)


def check_minimum(case, patches):
    """Assert the case's minimum counts on what the oracle made of it; returns the stage histogram."""
    h, r = histogram(p.stage for p in patches), result_histogram(patches)
    for s, m in case.minimum.items():
        assert h.get(s, 0) >= m, f"{case.name}: the oracle leaves {h.get(s, 0)} patches at stage {s}, the case needs {m}: {h}"
    for c, m in case.results.items():
        assert r.get(c, 0) >= m, f"{case.name}: NLopt returns {c} for {r.get(c, 0)} patches, the case needs {m}: {r}"
    return h


def oracle_refine(case, oracle_scene, seeds=None):
    from oracle import oracle as orc
    seeds = refine_seeds(case) if seeds is None else seeds
    return orc.optimize_batch(oracle_scene, orc.patches_from_seeds(seeds), which=orc.best_optimizer(),
                              options=apply_options(orc.default_options(), case.options), n_threads=8)


def oracle_seed_loop(case, oracle_scene, points=None):
    from oracle import oracle as orc
    xyz, off, img, start_level = seed_loop_points(case) if points is None else points
    return orc.init_patches(oracle_scene, xyz, off, img, start_level=start_level, which=orc.best_optimizer(),
                            options=apply_options(orc.default_options(), case.options), n_threads=8)


def oracle_expand(case, oracle_scene, inputs=None):
    from oracle import oracle as orc
    mode, par, cc, width, skip = expand_inputs(case, oracle_scene) if inputs is None else inputs
    return orc.expand_batch(oracle_scene, mode, par, cc, width, skip, which=orc.best_optimizer(),
                            options=apply_options(orc.default_options(), case.options), n_threads=8)


def acos_class(run):
    """`run()` again with the oracle's acos() correctly rounded, as the device's is: the number of patches that change in a
    compared field.  The device may differ from the oracle in those patches and in no other."""
    from oracle import oracle as orc
    base = run()
    orc.set_libm_mode(1)
    try:
        other = run()
    finally:
        orc.set_libm_mode(0)
    vb, vo = orc.patch_view(base), orc.patch_view(other)
    return sum(1 for k in range(len(base)) if any(vb[k][f].tobytes() != vo[k][f].tobytes() for f in COMPARED))


def all_cases():
    """(kind, case, run) for every case: run(oracle_scene) gives the oracle's patches."""
    return ([("refine", c, oracle_refine) for c in refine_cases()] + [("seed", c, oracle_seed_loop) for c in seed_loop_cases()] +
            [("expand", c, oracle_expand) for c in expand_cases()])


def main():
    """Print the table of the docstring."""
    from oracle import oracle as orc
    orc.build()
    oscs = {}
    for kind, c, run in all_cases():
        osc = oscs.setdefault(c.scene, orc.OracleScene(scene(c.scene)))
        inputs = expand_inputs(c, osc) if kind == "expand" else None     # parents chosen once, under the host's own acos
        P = run(c, osc, inputs)
        print(f"{kind:6s} {c.name:20s} {check_minimum(c, P)}  nlopt {result_histogram(P)}  acos {acos_class(lambda: run(c, osc, inputs))}")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
