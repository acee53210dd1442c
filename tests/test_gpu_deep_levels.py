"""The photometric kernels on pyramid levels 5 and 6 and on views of four sizes in one scene, against the CPU oracle
(tests/deep_level_inputs.py; tests/test_cpu_deep_level_inputs.py shows with the oracle alone that these inputs reach the paths).

With the default MAXLEVEL = 5 sampleTexture stops at level 4 and prep_from_view forms the level's address arithmetically from
the level-0 size; MAXLEVEL = 7 reaches levels 5 and 6, whose address is a load from the view's table.  The sizes here are odd
and even and differ between the views of a scene, so the level offsets (stated in the kernel and again where the views are
uploaded), the level widths w0 >> l and the limits of the bounding-box gate are exercised where they could disagree.

Tolerance: NONE, as everywhere in this project -- float bits.  The one exception is the known host-acos class of the
refinement (tests/test_gpu_random_scenes.py): at most one patch per seed set, and it must equal the oracle run with a correctly
rounded acos."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_level_inputs as dli

pytestmark = pytest.mark.gpu

OUT_FIELDS = ("ok", "center", "normal", "n_images", "images", "color", "fmin", "x", "nevals", "stage", "result")


@pytest.fixture(scope="module")
def D():
    from hpmvs_amd import api
    from oracle import oracle as orc
    if api.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    orc.build()
    scene = dli.make_scene()
    g = api.Scene(scene, device=0)
    d = dict(scene=scene, gpu=g, osc=orc.OracleScene(scene), og=dli.gpu_options(), oc=dli.oracle_options(),
             seeds={which: dli.make_seeds(scene, which) for which in dli.SEED_SETS})
    yield d
    g.close()


@pytest.fixture(scope="module")
def refined(D):
    """{seed set: (the batch refined on the GPU, the patches refined by the oracle)}."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    out = {}
    for which, seeds in D["seeds"].items():
        b = api.Batch.from_seeds(seeds)
        api.optimize_batch(D["gpu"], b, D["og"])
        P = orc.patches_from_seeds(seeds)
        orc.optimize_batch(D["osc"], P, which=orc.best_optimizer(), options=D["oc"], n_threads=min(16, os.cpu_count() or 1))
        out[which] = (b, P)
    return out


def test_pyramid_of_every_view_and_level(D):
    for v in range(D["scene"].n_views):
        for l in range(8):
            a, b = D["osc"].level(v, l), D["gpu"].level(v, l)
            assert a.shape == b.shape, (v, l, a.shape, b.shape)
            assert np.array_equal(a, b), f"view {v} level {l}: {(a != b).sum()} bytes differ"
    assert D["gpu"].level(0, 6).shape == (16, 20, 3) and D["gpu"].level(2, 7).shape == (9, 7, 3)


@pytest.mark.parametrize("which", list(dli.SEED_SETS))
def test_inccs_parity(D, which):
    from hpmvs_amd import api
    from oracle import oracle as orc
    seeds = D["seeds"][which]
    P = orc.patches_from_seeds(seeds)
    sampled = 0
    for ref_idx, robust in [(0, 0), (1, 1)]:
        idx = np.nonzero(seeds.n_images > ref_idx)[0]     # (setINCCs reads list[ref_idx])
        sub = api.Batch.from_seeds(seeds, idx)
        got = api.inccs_batch(D["gpu"], sub, ref_idx, robust, D["og"])
        for row, k in enumerate(idx):
            want = orc.inccs(D["osc"], P[int(k)], ref_idx, robust, D["oc"])
            assert np.array_equal(got[row, :len(want)], want), (which, ref_idx, robust, int(k), got[row, :len(want)], want)
            sampled += int(((want != 2.0) & (want != 0.0)).sum())
    print(f"seeds {which}: {sampled} entries came from two sampled windows")
    assert sampled >= {"5": 1680, "6": 170, "6c": 1985}[which]   # (the oracle alone gives 3362, 342 and 3971)


@pytest.mark.parametrize("which", list(dli.SEED_SETS))
def test_objective_parity_and_grab_counts(D, which):
    from hpmvs_amd import api
    from oracle import oracle as orc
    seeds = D["seeds"][which]
    idx = np.nonzero(seeds.n_images >= 2)[0]
    batch = api.Batch.from_seeds(seeds, idx)
    P = orc.patches_from_seeds(seeds, idx)
    rng = np.random.default_rng(11)
    x0 = np.array([orc.initial_parameters(D["osc"], P[k], D["oc"]) for k in range(len(idx))])
    evaluated = 0
    for trial in range(4):
        x = x0 + (rng.uniform(-1, 1, size=x0.shape) * np.array([0.3, 2.0, 2.0]) if trial else 0.0)
        f_gpu, g_gpu = api.objective_batch(D["gpu"], batch, x, D["og"])
        f_cpu = np.array([orc.objective_at(D["osc"], P[k], x[k], D["oc"]) for k in range(len(idx))])
        g_cpu = np.array([dli.objective_grabs(D["osc"], P[k], x[k], D["oc"]) for k in range(len(idx))])
        bad = np.nonzero(f_gpu != f_cpu)[0]
        assert len(bad) == 0, (which, trial, len(bad), idx[bad][:5], f_gpu[bad][:5], f_cpu[bad][:5])
        assert np.array_equal(g_gpu, g_cpu), (which, trial, np.nonzero(g_gpu != g_cpu)[0][:10])
        evaluated += int((f_cpu < 2.0).sum())
    print(f"seeds {which}: {evaluated} objective values below 2.0 over 4 points")
    assert evaluated >= {"5": 1090, "6": 180, "6c": 1200}[which]   # (the oracle alone gives 2186, 366 and 2400)


@pytest.mark.parametrize("which", list(dli.SEED_SETS))
def test_refinement_is_bit_identical(D, refined, which):
    from helpers import equals_gpu_with_correctly_rounded_acos
    b, P = refined[which]
    stage = np.array([p.stage for p in P])
    nevals = np.array([p.nevals for p in P])
    differing = set(np.nonzero(stage != b.stage)[0].tolist())
    for k in np.nonzero(b.ok)[0]:
        if not (np.array_equal(np.array(P[k].center[:], dtype=np.float32), b.center[k]) and
                np.array_equal(np.array(P[k].normal[:], dtype=np.float32), b.normal[k]) and
                list(P[k].images[:P[k].n_images]) == list(b.images[k, :b.n_images[k]]) and P[k].nevals == b.nevals[k]):
            differing.add(int(k))
    print(f"seeds {which}: refined {int(b.ok.sum())}, ran the optimiser {(nevals > 0).sum()}, differing {sorted(differing)}")
    assert len(differing) <= 1, (which, sorted(differing))
    for k in differing:
        assert equals_gpu_with_correctly_rounded_acos(D["osc"], D["oc"], D["seeds"][which], k, b), \
            (which, k, "differs from the oracle and does NOT equal it with a correctly rounded acos")
    # the floors of tests/test_cpu_deep_level_inputs.py, on the oracle's results
    if which == "5":
        assert (stage == 0).sum() >= 110 and (nevals > 0).sum() >= 111
    elif which == "6":
        assert (stage == 2).sum() >= 300
    else:
        assert (nevals > 0).sum() >= 12 and (stage == 0).sum() >= 10


def test_both_builds_of_the_kernel_on_level_5(D, refined, tmp_path):
    """The 29-slot and the 64-slot build of the refinement kernel (tests/test_gpu_optimize.py) share prep_from_view: the level-5
    seeds, tiled to 8 400 patches, through each build in a process of its own -- every output array byte-identical between the
    two, and equal on the first 600 to the in-process run that test_refinement_is_bit_identical compares with the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import deep_level_inputs as dli
from hpmvs_amd import api
scene = dli.make_scene()
seeds = dli.make_seeds(scene, "5")
g = api.Scene(scene)
b = api.Batch.from_seeds(seeds, np.tile(np.arange(len(seeds.scale)), 14))
api.optimize_batch(g, b, dli.gpu_options())
np.savez(sys.argv[1], **{k: getattr(b, k) for k in %r})
g.close()
''' % (root, os.path.join(root, "tests"), OUT_FIELDS)
    outs = {}
    for slots in ("29", "64"):
        f = str(tmp_path / f"slots{slots}.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, HPMVS_SLOTS=slots), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[slots] = np.load(f)
    for k in OUT_FIELDS:
        assert outs["29"][k].tobytes() == outs["64"][k].tobytes(), k
    assert outs["29"]["ok"].sum() >= 14 * 110
    b = refined["5"][0]
    for k in OUT_FIELDS:
        assert outs["64"][k][:b.n].tobytes() == getattr(b, k).tobytes(), k


@pytest.mark.parametrize("fine", [False, True], ids=["half_a_pixel", "around_the_limit"])
def test_border_sweeps(D, fine):
    """setINCCs at every position of the walks across a side of the bounding-box gate: the gate's decision is in the value
    (2.0 in the walked slot, or in every slot where the walked view is the reference image), so the limits 3 and W - 3, H - 3
    with W = w0 >> level on odd sizes, and the level's pixels, are pinned on both sides of each limit.  The fine walks of
    levels 5 and 6 stand on the limit itself (tests/test_cpu_deep_level_inputs.py): they tell `<` from `<=`."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    seeds, sweeps = dli.make_sweeps(D["scene"], fine=fine)
    got = api.inccs_batch(D["gpu"], api.Batch.from_seeds(seeds), 0, 0, D["og"])
    P = orc.patches_from_seeds(seeds)
    want = np.array([orc.inccs(D["osc"], P[k], 0, 0, D["oc"]) for k in range(len(P))])
    assert len(sweeps) == (16 if fine else 24)
    for s in sweeps:
        a, w = got[s.rows, :2], want[s.rows]
        bad = np.nonzero((a != w).any(axis=1))[0]
        assert len(bad) == 0, (dli.describe(s), "positions", bad[:10], a[bad[:3]], w[bad[:3]])
        refused = w[:, s.slot] == 2.0
        assert not refused[0] and refused[-1] and 64 <= refused.sum() <= s.count - 64, dli.describe(s)
        if s.slot == 1:   # (a walked reference image is not always seen by a second view; then only the decision shows)
            assert ((w[~refused] != 0.0) & (w[~refused] != 2.0)).any(axis=1).sum() >= 64, dli.describe(s)   # windows were compared


def _poisoned(seeds, idx):
    from hpmvs_amd import api
    b = api.Batch.from_seeds(seeds, idx)
    rng = np.random.default_rng(5)
    for name in ("ok", "color", "ncc", "fmin", "x", "result", "nevals", "stage", "ngrabs"):
        a = getattr(b, name)
        a[...] = rng.integers(1, 100, size=a.shape).astype(a.dtype)
    return b, {name: getattr(b, name).copy() for name in api.Batch.FIELDS}


def _unchanged(b, saved):
    return [name for name in saved if getattr(b, name).tobytes() != saved[name].tobytes()]


def test_level_options_out_of_range_are_refused(D):
    """check_batch_shape is all that keeps the level arithmetic inside a view's slab: MAXLEVEL >= 8 (HPMVS_MAX_LEVELS),
    MAXLEVEL < 1 and MINLEVEL > MAXLEVEL are HPMVS_ERR_ARG on every entry point that samples, nothing is written, and the
    scene serves a valid call afterwards."""
    from hpmvs_amd import api
    L = api.lib()
    seeds = D["seeds"]["5"]
    idx = np.arange(64)
    for field, value, word in (("MAXLEVEL", 8, b"MAXLEVEL"), ("MAXLEVEL", 0, b"MAXLEVEL"), ("MINLEVEL", 8, b"MINLEVEL")):
        o = dli.gpu_options()
        setattr(o, field, value)
        b, saved = _poisoned(seeds, idx)
        cb = b.c_struct()
        assert L.hpmvs_optimize_batch(D["gpu"].h, C.byref(o), C.byref(cb), 0, None) == -2, (field, value)   # HPMVS_ERR_ARG
        assert word in L.hpmvs_last_error(), L.hpmvs_last_error()
        assert _unchanged(b, saved) == [], (field, value)
        with pytest.raises(api.HpmvsError, match="error -2"):
            api.optimize_batch(D["gpu"], b, o)
        out = np.full((b.n, b.max_images), 7.0, np.float32)
        assert L.hpmvs_inccs_batch(D["gpu"].h, C.byref(o), C.byref(cb), 0, 0, out.ctypes.data, 0, None) == -2
        f = np.full(b.n, 7.0); g = np.full(b.n, 7, np.int32); x = np.zeros((b.n, 3))
        assert L.hpmvs_objective_batch(D["gpu"].h, C.byref(o), C.byref(cb), x.ctypes.data, f.ctypes.data, g.ctypes.data, 0, None) == -2
        assert (out == 7.0).all() and (f == 7.0).all() and (g == 7).all() and _unchanged(b, saved) == []
    o = dli.gpu_options()
    o.MINLEVEL = 7            # MINLEVEL == MAXLEVEL is in range
    b = api.Batch.from_seeds(seeds, idx)
    api.optimize_batch(D["gpu"], b, o)
    b = api.Batch.from_seeds(seeds, idx)
    api.optimize_batch(D["gpu"], b, D["og"])
    assert b.ok.sum() >= 5


def test_options_deeper_than_a_views_pyramid_are_refused(D):
    """Scene D's views again with 3 pyramid levels: MAXLEVEL = 5 would have prep_from_view form addresses of levels 3 and 4
    past the slab."""
    import copy
    from hpmvs_amd import api
    L = api.lib()
    shallow = copy.copy(D["scene"])
    shallow.max_level = 2
    sc = api.Scene(shallow, device=0)
    try:
        assert sc.view_levels == [3] * 8
        seeds = D["seeds"]["5"]
        o = api.default_options()
        assert o.MAXLEVEL == 5
        b, saved = _poisoned(seeds, np.arange(64))
        cb = b.c_struct()
        assert L.hpmvs_optimize_batch(sc.h, C.byref(o), C.byref(cb), 0, None) == -2
        assert b"exceeds the pyramid levels" in L.hpmvs_last_error()
        assert _unchanged(b, saved) == []
        out = np.full((b.n, b.max_images), 7.0, np.float32)
        assert L.hpmvs_inccs_batch(sc.h, C.byref(o), C.byref(cb), 0, 0, out.ctypes.data, 0, None) == -2
        assert b"exceeds the pyramid levels" in L.hpmvs_last_error() and (out == 7.0).all()
        o.MAXLEVEL = 3        # as deep as the pyramid: served
        b = api.Batch.from_seeds(seeds, np.arange(64))
        api.optimize_batch(sc, b, o)
        assert set(np.unique(b.stage)) <= set(range(0, 10))
    finally:
        sc.close()


def test_init_patches_at_start_level_5(D):
    """Scene::initPatches with START_LEVEL = 5 on the mixed-size views (the oracle alone refines 140 of the 400 points)."""
    from hpmvs_amd import api, synth
    from oracle import oracle as orc
    xyz, off, img = synth.make_nvm_points(D["scene"], 400, start_level=5)
    batch = api.init_patches_batch(D["gpu"], xyz, off, img, start_level=5, options=D["og"])
    P = orc.init_patches(D["osc"], xyz, off, img, start_level=5, options=D["oc"], n_threads=8)
    stage = np.array([p.stage for p in P])
    assert np.array_equal(stage, batch.stage), np.nonzero(stage != batch.stage)[0][:10]
    assert np.array_equal(stage == 0, batch.ok.astype(bool)) and (stage == 0).sum() >= 70
    for k in range(len(P)):
        p = P[k]
        assert np.array_equal(np.array(p.center[:], dtype=np.float32), batch.center[k]), k
        if p.stage < 10:
            assert np.float32(p.scale) == batch.scale[k], k
            if p.stage == 0 or p.stage == 12:
                assert np.array_equal(np.array(p.normal[:], dtype=np.float32), batch.normal[k]), k
                assert list(p.images[:p.n_images]) == list(batch.images[k, :batch.n_images[k]]), k
                assert p.stage != 0 or p.nevals == batch.nevals[k], k
