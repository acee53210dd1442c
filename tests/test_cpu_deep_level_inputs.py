"""The inputs of tests/test_gpu_deep_levels.py do reach the paths they are meant for: the oracle alone, on scene D
(tests/deep_level_inputs.py).  Conditions on the generator, not measurements of the product: a failure here means the
generator has to be tuned, never the condition.  The seeds are fixed, so each floor is about half of what the oracle gives:

    condition                                            seeds   measured                        floor
    grabs that pass their gates at level 5               "5"     1263 even-width, 979 odd-width  630, 490
    grabs that pass their gates at level 6               "6"     127 even-width, 209 odd-width   63, 104
    grabs that pass their gates at level 6               "6c"    1855 even-width, 535 odd-width  925, 265
    patches refined (stage 0)                            "5"     221 of 600                      110
    patches that ran the optimiser                       "5"     223                             111
    patches that fail at stage 2                         "6"     599 of 600                      300
    patches that ran the optimiser                       "6"     1                               -
    patches that ran the optimiser at level 6            "6c"    24 (21 refined)                 12 (10)
    NVM points refined by initPatches, START_LEVEL 5     -       140 of 400                      70
    fine walks with a position on the limit itself       -       13 of 16                        every side x level, side x parity

Over synth's whole seeding square level 6 reaches the optimiser once: set "6" covers level-6 refinement through setINCCs,
objective_fn and the stage-2 decision only.  Set "6c" (the same generator within 1.5 units of the scene centre, chosen with the
oracle alone) is what runs the optimiser on level-6 grabs.
Every border sweep holds both outcomes of the gate with a single flip between them, on the side it names."""
import time

import numpy as np
import pytest

import deep_level_inputs as dli


@pytest.fixture(scope="module")
def D():
    from oracle import oracle as orc
    orc.build()
    t0 = time.time()
    scene = dli.make_scene()
    print(f"scene D rendered in {time.time() - t0:.2f} s")
    return dict(scene=scene, osc=orc.OracleScene(scene), opts=dli.oracle_options())


def test_scene_shape(D):
    scene, osc = D["scene"], D["osc"]
    assert scene.n_views == 8 and scene.max_level == 7
    assert [(v.width, v.height) for v in scene.views] == dli.SIZES * 2
    assert all(v.f == 1.2 * v.width and v.rgb.shape == (v.height, v.width, 3) and v.rgb.dtype == np.uint8 for v in scene.views)
    assert all(c == [b for b in range(8) if b != a] for a, c in enumerate(scene.covis))
    assert osc.level(0, 6).shape == (16, 20, 3) and osc.level(0, 5).shape == (32, 40, 3) and osc.level(2, 7).shape == (9, 7, 3)
    assert osc.level(3, 5).shape == (32, 43, 3)      # an even width whose level-5 width is odd
    # the 8 x 8 blocks of the rendering are gone on the levels that are sampled: no two neighbouring columns agree everywhere
    for lvl in (5, 6):
        img = osc.level(1, lvl).astype(int)
        assert (np.abs(np.diff(img, axis=1)).sum(axis=(0, 2)) > 0).all() and img.std() > 10
    o = D["opts"]
    assert o.MAXLEVEL == 7 and o.MIN_IMAGES_PER_PATCH == 2


@pytest.mark.parametrize("which,floor_even,floor_odd", [("5", 630, 490), ("6", 63, 104), ("6c", 925, 265)])
def test_grabs_pass_their_gates_on_the_deep_levels(D, which, floor_even, floor_odd):
    from oracle import oracle as orc
    seeds = dli.make_seeds(D["scene"], which)
    level = dli.SEED_SETS[which][0]
    assert len(seeds.scale) == 600 and (seeds.n_images >= 2).sum() >= 590
    g = dli.grabs(D["osc"], orc.patches_from_seeds(seeds), D["opts"])
    odd = sum(1 for (_, _, v, ok, lvl) in g if ok and lvl == level and dli.odd_width(D["scene"], v))
    even = sum(1 for (_, _, v, ok, lvl) in g if ok and lvl == level and not dli.odd_width(D["scene"], v))
    failed = sum(1 for x in g if not x[3])
    print(f"seeds {which}: grabs passed at level {level}: {even} on even-width views, {odd} on odd-width views; {failed} failed")
    assert even >= floor_even and odd >= floor_odd and failed >= 100
    assert all(lvl <= 6 for (_, _, _, _, lvl) in g)


def test_refinement_on_the_deep_levels(D):
    from oracle import oracle as orc
    got = {}
    for which in dli.SEED_SETS:
        P = orc.patches_from_seeds(dli.make_seeds(D["scene"], which))
        orc.optimize_batch(D["osc"], P, options=D["opts"], n_threads=8)
        stage = np.array([p.stage for p in P]); nevals = np.array([p.nevals for p in P])
        got[which] = (stage, nevals)
        print(f"seeds {which}: stages {dict(zip(*np.unique(stage, return_counts=True)))}, ran the optimiser {(nevals > 0).sum()}")
    assert (got["5"][0] == 0).sum() >= 110 and (got["5"][1] > 0).sum() >= 111
    assert (got["6"][0] == 2).sum() >= 300
    assert (got["6c"][1] > 0).sum() >= 12 and (got["6c"][0] == 0).sum() >= 10


def test_objective_grab_counts_from_the_oracle(D):
    """dli.objective_grabs (the oracle's objective over two-image lists) counts what sampleTexture passes: at the start point,
    whose frame is the patch's own up to rounding, it agrees with orc.sample_texture on all but gate-edge cases."""
    from oracle import oracle as orc
    seeds = dli.make_seeds(D["scene"], "5")
    idx = np.nonzero(seeds.n_images >= 3)[0][:150]
    P = orc.patches_from_seeds(seeds, idx)
    same = total = 0
    for k in range(len(idx)):
        x0 = orc.initial_parameters(D["osc"], P[k], D["opts"])
        n = dli.objective_grabs(D["osc"], P[k], x0, D["opts"])
        oks = [orc.sample_texture(D["osc"], P[k], 0, j, D["opts"])[0] for j in range(P[k].n_images)]
        same += int(n == (sum(oks) if oks[0] else 0))
        total += n
        assert 0 <= n <= P[k].n_images
    print(f"objective grab counts: {same} of {len(idx)} equal sampleTexture's on the patch itself, {total} grabs in all")
    assert same >= 0.95 * len(idx) and total >= 150


def test_every_border_sweep_crosses_its_side_of_the_gate(D):
    from oracle import oracle as orc
    scene, osc, o = D["scene"], D["osc"], D["opts"]
    t0 = time.time()
    seeds, sweeps = dli.make_sweeps(scene)
    print(f"{len(sweeps)} sweeps of {dli.SWEEP_STEPS} patches built in {time.time() - t0:.2f} s")
    assert len(sweeps) == 24 and len(seeds.scale) == 24 * dli.SWEEP_STEPS
    P = orc.patches_from_seeds(seeds)
    covered = set()
    for s in sweeps:
        ok, geo = [], []
        for k in range(s.first, s.first + dli.SWEEP_STEPS):
            passed, _, lvl, g = orc.sample_texture(osc, P[k], 0, s.slot, o)
            ok.append(passed)
            if passed:
                assert lvl == s.level, dli.describe(s)
                geo.append(g)
        ok = np.array(ok)
        tag = dli.describe(s)
        assert ok[0] and not ok[-1] and (np.diff(ok.astype(int)) != 0).sum() == 1, tag     # inside -> outside, one flip
        assert 64 <= ok.sum() <= dli.SWEEP_STEPS - 64, tag                                # about half a pixel on either side
        geo = np.array(geo, dtype=np.float64)
        axis = dli.SIDES.index(s.side) % 2
        step = np.abs(np.diff(geo[:, axis]))      # the oracle's own projected centres: at most 1/256 level pixel apart
        assert step.max() <= 1.0 / 256 and step.min() > 0, (tag, step.max())
        # the last position that passes lies within a step of the limit of the named side and well inside the other three
        c, dx, dy = geo[-1, 0:2], geo[-1, 2:4], geo[-1, 4:6]
        corners = np.array([c + a * 3.5 * dx + b * 3.5 * dy for a in (-1, 1) for b in (-1, 1)])
        v = scene.views[s.view]
        W, H = v.width >> s.level, v.height >> s.level
        m = np.array([corners[:, 0].min() - 3, corners[:, 1].min() - 3, (W - 3) - corners[:, 0].max(), (H - 3) - corners[:, 1].max()])
        k = dli.SIDES.index(s.side)
        assert 0 <= m[k] < 1.5 / 256 and np.delete(m, k).min() > 0.2, (tag, m)
        if s.slot == 1:   # the reference image of these patches passes everywhere, so the walked slot alone decides its entry
            assert all(orc.sample_texture(osc, P[j], 0, 0, o)[0] for j in (s.first, s.first + dli.SWEEP_STEPS - 1)), tag
        covered.add((s.level, dli.odd_width(scene, s.view), s.side))
    assert covered == {(l, odd, side) for l in (0, 5, 6) for odd in (False, True) for side in dli.SIDES}
    assert {s.slot for s in sweeps} == {0, 1}
    assert {(scene.views[s.view].width >> s.level) % 2 for s in sweeps} == {0, 1}       # level widths of both parities


def test_fine_walks_stand_on_the_limit_itself(D):
    """The fine walks of levels 5 and 6 hold positions whose bounding-box edge EQUALS the limit in float32 (3 on the left and
    at the top, where the gate then passes; W - 3 and H - 3 on the right and at the bottom, where it fails): what tells `<` from
    `<=`.  Measured: 13 of the 16 walks hold one (1 to 17 positions each); the floor is one per side and level and one per
    side and width parity, which is what a comparison turned the other way has to meet to be seen."""
    from oracle import oracle as orc
    scene, osc, o = D["scene"], D["osc"], D["opts"]
    seeds, walks = dli.make_sweeps(scene, fine=True)
    assert len(walks) == 16 and len(seeds.scale) == 16 * dli.FINE_STEPS and {w.level for w in walks} == {5, 6}
    P = orc.patches_from_seeds(seeds)
    on_limit, hits = set(), 0
    for w in walks:
        v = scene.views[w.view]
        k = dli.SIDES.index(w.side)
        limit = np.float32([3, 3, (v.width >> w.level) - 3, (v.height >> w.level) - 3][k])
        ok, edge = [], []
        for j in range(w.first, w.first + w.count):
            passed, _, lvl, geo = orc.sample_texture(osc, P[j], 0, w.slot, o)
            e, geo2 = dli.window_edge(osc, P[j], w, o)
            assert not passed or (lvl == w.level and np.array_equal(geo, geo2)), dli.describe(w)
            ok.append(passed); edge.append(e)
        ok, edge = np.array(ok), np.array(edge, dtype=np.float32)
        # the named side alone decides along the walk, by sampleTexture's own comparison
        assert np.array_equal(ok, ~(edge < limit) if k < 2 else ~(edge >= limit)), dli.describe(w)
        assert ok[0] and not ok[-1] and 64 <= ok.sum() <= w.count - 64, dli.describe(w)
        if (edge == limit).any():
            on_limit.add((w.level, w.side)); on_limit.add((w.side, dli.odd_width(scene, w.view)))
            hits += 1
    print(f"{hits} of {len(walks)} fine walks hold a position on the limit itself")
    assert on_limit >= {(l, side) for l in (5, 6) for side in dli.SIDES} | {(side, odd) for side in dli.SIDES for odd in (False, True)}


def test_init_patches_refines_at_start_level_5(D):
    from hpmvs_amd import synth
    from oracle import oracle as orc
    xyz, off, img = synth.make_nvm_points(D["scene"], 400, start_level=5)
    P = orc.init_patches(D["osc"], xyz, off, img, start_level=5, options=D["opts"], n_threads=8)
    stage = np.array([p.stage for p in P])
    print(f"initPatches at START_LEVEL 5: stages {dict(zip(*np.unique(stage, return_counts=True)))}")
    assert (stage == 0).sum() >= 70 and (stage == 2).sum() >= 50 and np.diff(off).max() <= 8
