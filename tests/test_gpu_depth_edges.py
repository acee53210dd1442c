"""The depth-map entry points (kernel_depth.hip: set_depths, depth_gates, depth_footprints, depth_ops, level_support) against
the oracle on the scenes of tests/depth_edge_inputs.py: 70 views of six sizes (a second, partly filled chunk of lanes; odd
maps; levels with 0 rows), 8 pyramid levels, lists of up to 256 ids, patches on the image borders, outside, behind a camera
and with levels outside the pyramid.  The oracle runs on EVERY patch; every comparison is exact.  No refinement kernel runs.
(tests/test_cpu_depth_edge_inputs.py shows on the oracle alone that these inputs reach those paths.)"""
import numpy as np
import pytest

import depth_edge_inputs as dei

pytestmark = pytest.mark.gpu

SCENES = ["A", "B"]


class _Case:
    pass


@pytest.fixture(scope="module")
def cases():
    from hpmvs_amd import api
    from oracle import oracle as orc
    if api.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    orc.build()
    out = {}
    for which in SCENES:
        c = _Case()
        c.which = which
        c.scene = dei.make_scene(which)
        c.osc = orc.OracleScene(c.scene)
        c.gpu = api.Scene(c.scene, device=0)
        c.n_levels = c.scene.max_level + 1
        c.V = c.scene.n_views
        c.P = dei.make_patches(c.scene, which)
        c.O = c.P.oracle()
        c.batch = c.P.batch()
        c.shapes = dei.map_shapes(c.osc, c.n_levels)
        c.sizes0 = [(v.width, v.height) for v in c.scene.views]
        c.setters = dei.setters(c.osc, c.P)
        c.all = np.arange(c.P.n)
        out[which] = c
    yield out
    for c in out.values():
        c.gpu.close()


def _maps_differ(c, D):
    """None, or the first (view, level, cells that differ) between the device's maps and the oracle's."""
    from hpmvs_amd import api
    for (v, l) in sorted(c.shapes):
        g, o = api.depth_level(c.gpu, v, l), D.level(v, l)
        if g.shape != o.shape or not np.array_equal(g, o):
            return (v, l, g.shape, o.shape, int((g != o).sum()) if g.shape == o.shape else -1)
    return None


def _gates_equal(c, D, margin, abs_int):
    from hpmvs_amd import api
    v, b, f = api.depth_gates_batch(c.gpu, c.batch, margin, abs_int)
    got = np.stack([v, b, f], axis=1)
    want = dei.gates(D, c.O, c.all, margin, abs_int)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (c.which, margin, abs_int, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
    return got


def _enter(c, D, idx):
    """setDepths of the patches idx on both sides (device: one set_depths_batch with ok = 1 on them)."""
    from hpmvs_amd import api
    for k in idx:
        D.set_depths(c.O[int(k)])
    c.batch.ok[:] = 0
    c.batch.ok[idx] = 1
    api.set_depths_batch(c.gpu, c.batch)
    c.batch.ok[:] = 0


@pytest.mark.parametrize("which", SCENES)
def test_shapes_and_reset(cases, which):
    from hpmvs_amd import api
    c = cases[which]
    api.depth_reset(c.gpu)
    cells = 0
    for (v, l), shape in c.shapes.items():
        g = api.depth_level(c.gpu, v, l)
        assert g.shape == shape, (v, l, g.shape, shape)
        assert (g == dei.MAX_DEPTH).all(), (v, l)
        cells += g.size
    assert cells == sum(a * b for a, b in c.shapes.values()) > 0
    assert any(a * b == 0 for a, b in c.shapes.values())


@pytest.mark.parametrize("which", SCENES)
def test_gates_on_empty_maps(cases, which):
    from hpmvs_amd import api
    from oracle import oracle as orc
    c = cases[which]
    api.depth_reset(c.gpu)
    D = orc.OracleDepths(c.osc)
    for abs_int in (0, 1):
        got = _gates_equal(c, D, 1.0, abs_int)
        assert got[:, 1].max() == 0 and got[:, 0].max() > 64 and got[:, 2].max() > 64


@pytest.mark.parametrize("which", SCENES)
def test_set_depths_and_gates_on_written_maps(cases, which):
    """setDepths of every second setter; then of the non-setters alone, which changes nothing: the device skips a (patch,
    image) pair with a negative depth (the reference CHECK-fails there, Scene.cpp:363), and the other images of these
    patches -- they lie behind the ring of cameras -- see them outside their maps (the oracle, asked to enter only their
    pairs with a positive depth, says so)."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    c = cases[which]
    api.depth_reset(c.gpu)
    D = orc.OracleDepths(c.osc)
    _enter(c, D, np.nonzero(c.setters)[0][::2])
    assert _maps_differ(c, D) is None, _maps_differ(c, D)
    assert dei.n_written(D, c.shapes) >= 1000
    assert all((D.level(*key) >= 0).all() for key in c.shapes)
    before = dei.oracle_maps(D, c.shapes)
    non = np.nonzero(~c.setters)[0]
    assert len(non) >= 100
    z = dei.attached_depths(c.osc, c.P)
    pos = c.P.take(non)
    for j in range(pos.n):
        m = int(pos.n_images[j])
        ids = pos.images[j, :m][z[non[j], :m] > 0]
        pos.images[j] = -1
        pos.images[j, :len(ids)] = ids
        pos.n_images[j] = len(ids)
    assert (pos.n_images < c.P.n_images[non]).all() and (pos.n_images > 0).sum() >= 50
    PO = pos.oracle()
    for j in range(pos.n):
        D.set_depths(PO[j])
    assert all(np.array_equal(before[key], D.level(*key)) for key in c.shapes)
    c.batch.ok[non] = 1
    api.set_depths_batch(c.gpu, c.batch)
    c.batch.ok[:] = 0
    assert _maps_differ(c, D) is None, _maps_differ(c, D)
    for margin in (1.0, 0.05):
        for abs_int in (0, 1):
            _gates_equal(c, D, margin, abs_int)


@pytest.mark.parametrize("which", SCENES)
def test_gates_on_random_maps(cases, which):
    from hpmvs_amd import api
    from oracle import oracle as orc
    c = cases[which]
    api.depth_reset(c.gpu)
    D = orc.OracleDepths(c.osc)
    fill = dei.random_fill(c.shapes, 101)
    dei.fill_oracle(D, fill)
    dei.fill_gpu(c.gpu, fill)
    assert _maps_differ(c, D) is None
    for margin in (1.0, 0.05):
        for abs_int in (0, 1):
            got = _gates_equal(c, D, margin, abs_int)
    assert (got[:, 1] > 0).any()


@pytest.mark.parametrize("which", SCENES)
def test_ordered_depth_ops_equal_the_sequential_loop(cases, which):
    """4 000 setDepths(patch, subtract) calls over the setters and copies of them moved +-0.05 % along the ray of their first
    image (another depth in the same cell, where the order decides), 40 % subtractions, 100 calls not made."""
    from hpmvs_amd import api
    from oracle import oracle as orc
    c = cases[which]
    rng = np.random.default_rng(7)
    base = c.P.take(np.nonzero(c.setters & (c.P.n_images > 0))[0])
    cams = np.array([c.scene.views[int(base.images[k, 0])].c for k in range(base.n)], dtype=np.float64)
    fac = rng.choice([0.9995, 1.0005], size=base.n)
    moved = base.take(np.arange(base.n))
    moved.center[:, :3] = (cams + (base.center[:, :3].astype(np.float64) - cams) * fac[:, None]).astype(np.float32)
    still = dei.setters(c.osc, moved)
    assert still.sum() > base.n // 2
    moved = moved.take(np.nonzero(still)[0])
    pool = dei.Patches(*[np.concatenate([getattr(base, f), getattr(moved, f)]) for f in ("center", "normal", "scale", "n_images", "images")])
    ops = pool.take(rng.integers(0, pool.n, size=4000))
    sub = (rng.random(ops.n) < 0.4).astype(np.uint8)
    b = ops.batch()
    b.ok[:] = 1
    b.ok[rng.choice(ops.n, size=100, replace=False)] = 0
    api.depth_reset(c.gpu)
    api.depth_ops_batch(c.gpu, b, sub)
    O = ops.oracle()
    D = orc.OracleDepths(c.osc)
    for t in range(ops.n):
        if b.ok[t]:
            D.set_depths(O[t], subtract=bool(sub[t]))
    assert _maps_differ(c, D) is None, _maps_differ(c, D)
    # the sequence did meet cells with several depths and did clear cells: the maps are not those of the sets alone
    D2 = orc.OracleDepths(c.osc)
    for t in range(ops.n):
        if b.ok[t] and not sub[t]:
            D2.set_depths(O[t])
    n_set, n_set_without = dei.n_written(D, c.shapes), dei.n_written(D2, c.shapes)
    assert 0 < n_set < n_set_without
    assert not all(np.array_equal(D.level(*key), D2.level(*key)) for key in c.shapes)
    assert _maps_differ(c, D2) is not None


@pytest.mark.parametrize("which", SCENES)
def test_level_support(cases, which):
    from hpmvs_amd import api
    from oracle import oracle as orc
    c = cases[which]
    for m in range(-1, 9):
        got = api.level_support_batch(c.gpu, c.batch, m)
        want = np.array([orc.level_support(c.osc, c.O[k], m) for k in range(c.P.n)], dtype=np.int32)
        assert np.array_equal(got, want), (which, m, int((got != want).sum()))


@pytest.fixture(scope="module")
def footprints(cases):
    """One depth_footprints_batch call per scene; everything the tests below do with it runs on the CPU."""
    from hpmvs_amd import api
    out = {}
    for which, c in cases.items():
        api.depth_reset(c.gpu)
        out[which] = api.depth_footprints_batch(c.gpu, c.batch)
    return out


@pytest.mark.parametrize("which", SCENES)
def test_footprint_writes(cases, footprints, which):
    from oracle import oracle as orc
    c = cases[which]
    wr = footprints[which][0]
    assert wr.shape == (c.P.n, dei.MAX_IMAGES, 4)
    used = np.arange(dei.MAX_IMAGES)[None, :] < c.P.n_images[:, None]
    assert (wr[~used][:, 0] == -1).all()
    D = orc.OracleDepths(c.osc)
    some = np.nonzero(c.setters & (c.P.n_images > 0))[0]
    some = np.concatenate([some[:270], some[c.P.n_images[some] > 64][:30]])
    views = dei.map_views(D, c.shapes)
    n_cells = 0
    for k in some[:300]:
        D.set_depths(c.O[int(k)])
        want = dei.written_cells(views)
        rows = wr[k][wr[k][:, 0] >= 0]
        got = {tuple(int(t) for t in r) for r in rows}
        assert got == want, (which, int(k), sorted(got ^ want)[:4])
        D.set_depths(c.O[int(k)], subtract=True)
        assert dei.n_written(views, c.shapes) == 0, (which, int(k))
        n_cells += len(want)
    assert len(some) == 300 and n_cells > 300
    # a row whose depth would be negative names no cell
    z = dei.attached_depths(c.osc, c.P)
    neg = z < 0
    assert neg.sum() >= 50 and (wr[neg][:, 0] == -1).all()
    # ... and every row that names a cell names one of its own view, inside that view's map
    rows = wr[wr[:, :, 0] >= 0]
    assert np.array_equal(rows[:, 0], c.P.images[wr[:, :, 0] >= 0])
    cols = np.array([[c.shapes[(v, l)][0] for l in range(c.n_levels)] for v in range(c.V)])
    rws = np.array([[c.shapes[(v, l)][1] for l in range(c.n_levels)] for v in range(c.V)])
    assert ((rows[:, 1] >= 0) & (rows[:, 1] < c.n_levels)).all()
    assert ((rows[:, 2] >= 0) & (rows[:, 2] < cols[rows[:, 0], rows[:, 1]]) & (rows[:, 3] >= 0) & (rows[:, 3] < rws[rows[:, 0], rows[:, 1]])).all()


def reads_changed(c, fp, n=600, with_view_block=True, with_frees=True):
    """How many of the first n patches change an oracle count when only the cells their footprints name keep the content of
    fill 1 and every other cell of every map holds an independent fill 2."""
    from oracle import oracle as orc
    _, fr, at, vb = fp
    fill1, fill2 = dei.random_fill(c.shapes, 101), dei.random_fill(c.shapes, 202)
    D = orc.OracleDepths(c.osc)
    dei.fill_oracle(D, fill1)
    want = dei.gates(D, c.O, np.arange(n))
    M = dei.MixedMaps(D, c.shapes, fill1, fill2)
    changed = 0
    for k in range(n):
        cells = dei.read_cells(c.shapes, c.sizes0, c.n_levels, fr[k], at[k], vb[k], with_view_block, with_frees)
        changed += int(tuple(want[k]) != M.counts_with(cells, c.O[k]))
    return changed


@pytest.mark.parametrize("which", SCENES)
def test_footprint_reads(cases, footprints, which):
    """The gates of a patch read no cell its footprints do not name: with every other cell of every map replaced, patch by
    patch, the oracle's three counts stay.  (That this check can fail was checked once on the CPU: with the view_block blocks
    left out of the kept cells 171 of the 600 patches of scene A change a count and 39 of scene B; with the frees cells left
    out 64 and 58.)"""
    c = cases[which]
    _, fr, at, vb = footprints[which]
    assert fr.shape == (c.P.n, dei.MAX_IMAGES, 4) and at.shape == (c.P.n, dei.MAX_IMAGES, 3) and vb.shape == (c.P.n, c.V, 3)
    used = np.arange(dei.MAX_IMAGES)[None, :] < c.P.n_images[:, None]
    assert (fr[~used][:, 0] == -1).all() and (at[~used][:, 0] == -1).all()
    assert np.array_equal(at[used][:, 0], c.P.images[used]) and np.isin(vb[:, :, 0], (0, 1)).all()
    assert (vb[:, 64:, 0] == 1).any() or c.V <= 64
    assert reads_changed(c, footprints[which]) == 0
