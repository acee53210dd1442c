"""The device against the oracle on inputs that REACH the late rejection stages (tests/stage_inputs.py; what the oracle makes
of them is pinned on the CPU by tests/test_cpu_stage_inputs.py): assureImageAngles failing before and after the optimiser
(3, 8), filterImagesNCC failing behind the optimiser and behind setRefImage (6, 9), filterImagesByAngle on the gate's edge (7),
optimizePatch failing by image count and by NLopt's ROUNDOFF_LIMITED (4), and the exits of the seed loop (10, 11, 12) and of
the expansion (20, 22) around them.  Through api.optimize_batch, both builds of the kernel, the open batch behind single-patch
callers, other batch compositions, api.init_patches_batch and api.expand_batch.

No tolerance: every comparison is equality of bytes.  A failed patch comes back untouched, also when it failed behind a
completed optimiser run.  The one exemption is the host-acos class of tests/test_gpu_random_scenes.py: at most one differing
patch per refine case, and it must equal the oracle run again with a correctly rounded acos()."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_inputs as si

pytestmark = pytest.mark.gpu

FIELDS = ("ok", "center", "normal", "scale", "n_images", "images", "color", "ncc", "fmin", "x", "result", "nevals", "stage", "ngrabs")
REFINE = {c.name: c for c in si.refine_cases()}


@pytest.fixture(scope="module")
def world():
    """Scenes on both sides, made on first use and shared by the tests of this module."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    if api.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    orc.build()
    assert orc.best_optimizer() == orc.OPT_REF

    class World:
        def __init__(self):
            self.gpu, self.osc, self.refined = {}, {}, {}

        def scenes(self, name):
            if name not in self.gpu:
                self.gpu[name] = api.Scene(si.scene(name), device=0)
                self.osc[name] = orc.OracleScene(si.scene(name))
            return self.gpu[name], self.osc[name]

        def refine(self, name):
            """(seeds, the oracle's patches, the device's batch) of a refine case, computed once."""
            if name not in self.refined:
                case = REFINE[name]
                g, osc = self.scenes(case.scene)
                seeds = si.refine_seeds(case)
                b = api.Batch.from_seeds(seeds)
                api.optimize_batch(g, b, si.apply_options(api.default_options(), case.options))
                self.refined[name] = (seeds, si.oracle_refine(case, osc, seeds), b)
            return self.refined[name]

    w = World()
    yield w
    for g in w.gpu.values():
        g.close()


def images_equal(n_a, img_a, n_b, img_b):
    """Per row: the same count and the same ids in the first `count` slots."""
    m = min(img_a.shape[1], img_b.shape[1])
    assert n_a.max(initial=0) <= m and n_b.max(initial=0) <= m
    used = np.arange(m)[None, :] < n_a[:, None]
    return (n_a == n_b) & ((img_a[:, :m] == img_b[:, :m]) | ~used).all(axis=1)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(REFINE))
def test_refine_case_matches_the_oracle(name, world):
    from oracle import oracle as orc
    from helpers import equals_gpu_with_correctly_rounded_acos
    case = REFINE[name]
    seeds, P, b = world.refine(name)
    pv = orc.patch_view(P)
    hist = si.check_minimum(case, P)
    print(f"{name}: oracle stages {hist}, nlopt {si.result_histogram(P)}; device stages {si.histogram(b.stage)}, "
          f"results {si.histogram(b.result[b.nevals > 0])}")
    ok = b.ok.astype(bool)
    # a failed patch is untouched, whatever stage it failed at -- no exemption
    bad = ~ok
    assert same_bytes(b.center[bad], seeds.center[bad]) and same_bytes(b.normal[bad], seeds.normal[bad])
    assert same_bytes(b.n_images[bad], seeds.n_images[bad]) and same_bytes(b.images[bad], seeds.images[bad])
    assert same_bytes(b.scale, seeds.scale)
    assert np.array_equal(ok, b.stage == 0)
    assert np.all(b.ncc[ok] == np.float32(1.4))
    # against the oracle, per patch
    differs = (pv["stage"] != b.stage) | (pv["nlopt_result"] != b.result) | (pv["nevals"] != b.nevals)
    differs |= pv["fmin"].view(np.uint64) != b.fmin.view(np.uint64)
    good = ok & (pv["stage"] == 0)
    same_patch = ((pv["center"].view(np.uint32) == b.center.view(np.uint32)).all(axis=1) &
                  (pv["normal"].view(np.uint32) == b.normal.view(np.uint32)).all(axis=1) &
                  (pv["color"].view(np.uint32) == b.color.view(np.uint32)).all(axis=1) &
                  images_equal(pv["n_images"], pv["images"], b.n_images, b.images))
    differs |= good & ~same_patch
    differing = np.nonzero(differs)[0].tolist()
    print(f"{name}: differing patches (allowed: one, of the host-acos class): {differing}")
    assert len(differing) <= 1, (name, differing, pv["stage"][differing], b.stage[differing])
    oc = si.apply_options(orc.default_options(), case.options)
    for k in differing:
        assert equals_gpu_with_correctly_rounded_acos(world.scenes(case.scene)[1], oc, seeds, k, b), \
            (name, k, "differs from the oracle and does NOT equal it with a correctly rounded acos")
    if not differing:
        for s, m in case.minimum.items():   # what this run covered ON THE DEVICE
            assert (b.stage == s).sum() >= m, (name, s)


def test_the_refine_cases_cover_the_late_stages_on_the_device(world):
    best = collections.Counter()
    for name in REFINE:
        for s, c in si.histogram(world.refine(name)[2].stage).items():
            best[s] = max(best[s], c)
    print("most patches per stage over the refine cases, on the device:", dict(sorted(best.items())))
    assert all(best[s] >= m for s, m in si.REFINE_REQUIRED.items()), best


CHILD = r'''
import sys, numpy as np
sys.path[:0] = [%r, %r]
import stage_inputs as si
from hpmvs_amd import api
si.load_scenes(sys.argv[2])   # the parent's rendered views
out, scenes = {}, {}
for case in si.refine_cases():
    if case.scene not in scenes:
        scenes[case.scene] = api.Scene(si.scene(case.scene), device=0)
    seeds = si.refine_seeds(case)
    n = len(seeds.scale)
    b = api.Batch.from_seeds(seeds, np.tile(np.arange(n), -(-4000 // n)))   # a few thousand patches: every wavefront of several workgroups in use
    api.optimize_batch(scenes[case.scene], b, si.apply_options(api.default_options(), case.options))
    for f in %r:
        out[case.name + "." + f] = getattr(b, f)
np.savez(sys.argv[1], **out)
'''


def test_both_builds_of_the_kernel_on_the_late_stages(world, tmp_path):
    """The 29-slot and the 64-slot build of the refinement kernel (tests/test_gpu_optimize.py,
    test_both_builds_of_the_kernel_give_the_same_results), forced with HPMVS_SLOTS in one fresh process each, on every refine
    case tiled to 4000 patches and more: every output array byte-identical between the builds, every tile equal to the
    in-process run that the tests above compare with the oracle."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD % (os.path.dirname(here), here, FIELDS)
    outs = {}
    rendered = str(tmp_path / "scenes.pickle")
    si.save_scenes(rendered)
    for slots in ("29", "64"):
        f = str(tmp_path / f"slots{slots}.npz")
        r = subprocess.run([sys.executable, "-c", code, f, rendered], env=dict(os.environ, HPMVS_SLOTS=slots), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[slots] = np.load(f)
    assert sorted(outs["29"].files) == sorted(outs["64"].files) == sorted(f"{c}.{f}" for c in REFINE for f in FIELDS)
    for k in outs["29"].files:
        assert same_bytes(outs["29"][k], outs["64"][k]), k
    seen = collections.Counter()
    for name in REFINE:
        b = world.refine(name)[2]
        reps = -(-4000 // b.n)
        for f in FIELDS:
            tiled, mine = outs["64"][f"{name}.{f}"], getattr(b, f)
            assert tiled.shape[0] == reps * b.n
            assert same_bytes(tiled, np.concatenate([mine] * reps)), (name, f)
        for s, c in si.histogram(outs["29"][f"{name}.stage"]).items():
            seen[s] += c
    print("stages over the tiled cases, per build:", dict(sorted(seen.items())))
    # every case has at most 400 patches, so it is tiled ten times or more: ten times what the case set has to reach
    assert all(seen[s] >= 10 * m for s, m in si.REFINE_REQUIRED.items()), seen


@pytest.mark.parametrize("name", ["min_angle_40", "set_ref_image"])
def test_single_patch_callers_on_the_late_stages(name, world):
    """One patch per call goes through the open batch: every patch of the case that ends at 3, 6, 8 or 9, and 20 that succeed,
    equal their row of the batch result in every field."""
    from hpmvs_amd import api
    case = REFINE[name]
    seeds, _, b = world.refine(name)
    g = world.scenes(case.scene)[0]
    o = si.apply_options(api.default_options(), case.options)
    late = np.nonzero(np.isin(b.stage, (3, 6, 8, 9)))[0]
    idx = np.concatenate([late, np.nonzero(b.stage == 0)[0][:20]])
    print(f"{name}: single-patch calls at stages {si.histogram(b.stage[idx])}")
    assert len(late) >= 10 and (b.stage[idx] == 0).sum() == 20
    for j in idx:
        one = api.Batch.from_seeds(seeds, np.array([j]))
        api.optimize_batch(g, one, o)
        for f in FIELDS:
            assert same_bytes(getattr(one, f)[0], getattr(b, f)[j]), (name, int(j), int(b.stage[j]), f)


def test_batch_composition_on_the_late_stages(world):
    """The MIN_ANGLE 40 deg case in reversed order and as two halves: the same bytes per patch."""
    from hpmvs_amd import api
    case = REFINE["min_angle_40"]
    seeds, _, b = world.refine(case.name)
    g = world.scenes(case.scene)[0]
    o = si.apply_options(api.default_options(), case.options)
    n = b.n
    for idx in (np.arange(n)[::-1], np.arange(n // 2), np.arange(n // 2, n)):
        part = api.Batch.from_seeds(seeds, idx)
        api.optimize_batch(g, part, o)
        assert {3, 8} <= set(part.stage.tolist())
        for f in FIELDS:
            assert same_bytes(getattr(part, f), getattr(b, f)[idx]), f


def test_seed_loop_matches_the_oracle_on_every_exit(world):
    """api.init_patches_batch against orc.init_patches, field by field as test_init_patches_batch_matches_oracle compares them,
    on points that end at 10, 11 and 12 and, under MIN_ANGLE 40 deg, at 3 and 8 inside the seed loop."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    (case,) = si.seed_loop_cases()
    g, osc = world.scenes(case.scene)
    points = si.seed_loop_points(case)
    xyz, off, img, start_level = points
    P = si.oracle_seed_loop(case, osc, points)
    pv = orc.patch_view(P)
    hist = si.check_minimum(case, P)
    b = api.init_patches_batch(g, xyz, off, img, start_level=start_level, options=si.apply_options(api.default_options(), case.options))
    print(f"{case.name}: oracle stages {hist}; device stages {si.histogram(b.stage)}")
    assert np.array_equal(pv["stage"], b.stage), np.nonzero(pv["stage"] != b.stage)[0][:10]
    assert np.array_equal(b.ok.astype(bool), b.stage == 0)
    for s, m in {**si.SEED_LOOP_REQUIRED, **case.minimum}.items():
        assert (b.stage == s).sum() >= m, s
    # every row: the centre ((float)xyz where no seed was refined); the seed's scale, normal and list where one was built
    # (unchanged by a refinement that failed), the refined ones at 0 and 12; zeros where none was built
    assert same_bytes(pv["center"], b.center)
    assert same_bytes(pv["scale"], b.scale)
    assert same_bytes(pv["normal"], b.normal)
    assert images_equal(pv["n_images"], pv["images"], b.n_images, b.images).all()
    built = ~np.isin(b.stage, (10, 11))
    assert (b.n_images[~built] == 0).all() and (b.scale[~built] == 0).all() and (b.n_images[built] >= 2).all()


@pytest.mark.parametrize("case", si.expand_cases(), ids=lambda c: c.name)
def test_expansion_matches_the_oracle_on_the_late_stages(case, world):
    """api.expand_batch against orc.expand_batch with the case's options, per candidate as test_expand_matches_oracle compares
    them; candidates end at 3 and 8 beside 0, 2, 20 and 22."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    g, osc = world.scenes(case.scene)
    inputs = si.expand_inputs(case, osc)
    mode, par, cc, width, skip = inputs
    ref = si.oracle_expand(case, osc, inputs)
    rv, pp = orc.patch_view(ref), orc.patch_view(par)
    hist = si.check_minimum(case, ref)
    parents = api.Batch(pp["center"], pp["normal"], pp["scale"], pp["n_images"], pp["images"][:, :32])
    assert pp["n_images"].max() <= 32
    out = api.expand_batch(g, mode, parents, cc, width, skip, si.apply_options(api.default_options(), case.options))
    print(f"{case.name}: oracle stages {hist}; device stages {si.histogram(out.stage)}")
    assert out.n == len(ref) == len(par) * (6 if mode == 0 else 4)
    assert np.array_equal(rv["stage"], out.stage), np.nonzero(rv["stage"] != out.stage)[0][:10]
    assert np.array_equal(out.ok.astype(bool), out.stage == 0)
    for s, m in {**si.EXPAND_REQUIRED, **case.minimum}.items():
        assert (out.stage == s).sum() >= m, s
    # every candidate: the constructed (where it failed) or refined centre, normal and scale; the list of an accepted one
    assert same_bytes(rv["center"], out.center) and same_bytes(rv["normal"], out.normal) and same_bytes(rv["scale"], out.scale)
    acc = out.stage == 0
    assert images_equal(rv["n_images"][acc], rv["images"][acc], out.n_images[acc], out.images[acc]).all()
    if mode == 0:
        assert (out.stage[skip.astype(bool)] == 20).all()
