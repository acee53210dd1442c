"""The inputs of tests/test_gpu_depth_edges.py do reach the paths they are meant for: the oracle alone, on both scenes
(tests/depth_edge_inputs.py).  Conditions on the generator, not measurements of the product: a failure here means the
generator has to be tuned, never the condition."""
import numpy as np
import pytest

import depth_edge_inputs as dei


@pytest.fixture(scope="module")
def inputs():
    from oracle import oracle as orc
    orc.build()
    out = {}
    for which in ("A", "B"):
        scene = dei.make_scene(which)
        osc = orc.OracleScene(scene)
        P = dei.make_patches(scene, which)
        n_levels = scene.max_level + 1
        out[which] = dict(scene=scene, osc=osc, P=P, O=P.oracle(), n_levels=n_levels, shapes=dei.map_shapes(osc, n_levels),
                          setters=dei.setters(osc, P))
    return out


def _entered(inp):
    """Fresh oracle maps after set_depths of every second setter."""
    from oracle import oracle as orc
    D = orc.OracleDepths(inp["osc"])
    for k in np.nonzero(inp["setters"])[0][::2]:
        D.set_depths(inp["O"][int(k)])
    return D


def test_scene_shapes():
    A, B = dei.make_scene("A"), dei.make_scene("B")
    assert A.n_views == 70 and A.max_level == 5 and B.n_views == 5 and B.max_level == 7
    assert [(v.width, v.height) for v in A.views[:6]] == dei.SIZES["A"] and (A.views[69].width, A.views[69].height) == (91, 61)
    assert all(v.f == 1.2 * v.width and v.rgb.shape == (v.height, v.width, 3) and v.rgb.dtype == np.uint8 for v in A.views + B.views)
    assert all(c == [] for c in A.covis + B.covis)


def test_maps_have_odd_sizes_and_empty_levels(inputs):
    shapes = inputs["A"]["shapes"]
    # (cols, rows): 45x37 -> 22x18 at level 0 (the last pixel column and row have no cell), 1x1 pixels -> 0x0 cells at level 5
    assert shapes[(0, 0)] == (22, 18) and shapes[(0, 1)] == (11, 9) and shapes[(0, 5)] == (0, 0)
    assert shapes[(5, 5)] == (2, 0) and shapes[(4, 4)] == (1, 1)        # 128x35: 4x1 pixels; 33x33: 2x2 pixels
    assert any(c % 2 or r % 2 for (c, r) in shapes.values()) and any(c * r == 0 for (c, r) in shapes.values())
    assert len({shapes[(v, 0)] for v in range(70)}) == 6                # six sizes in one scene
    assert len(inputs["B"]["shapes"]) == 5 * 8 and inputs["B"]["shapes"][(0, 7)] == (0, 0) and inputs["B"]["shapes"][(1, 6)] == (1, 1)


def test_patches_cover_the_edges_of_the_rules(inputs):
    for which in ("A", "B"):
        inp = inputs[which]
        P, osc = inp["P"], inp["osc"]
        assert P.n == 1500 and P.images.shape == (1500, 256)
        assert np.isfinite(P.center).all() and np.isfinite(P.normal).all() and np.isfinite(P.scale).all()
        used = np.arange(256)[None, :] < P.n_images[:, None]
        assert ((P.images >= 0) & (P.images < osc.n_views))[used].all() and (P.images[~used] == -1).all()
        for m in dei.LIST_LENGTHS:
            assert (P.n_images == m).sum() >= 20, (which, int(m))
        z = dei.attached_depths(osc, P)
        assert ((z < 0).any(axis=1)).sum() >= 50, which                 # a negative depth in an attached view
        assert 100 <= (~inp["setters"]).sum() <= 400 and not (z == 0).any(), which
        # the rounded level of an attached view: below 0, every level of the pyramid, at or above n_levels
        from oracle import oracle as orc
        sup = np.array([[orc.level_support(osc, inp["O"][k], m) for m in (-1, inp["n_levels"] - 1)] for k in range(P.n)])
        assert ((sup[:, 0] < P.n_images).sum() >= 50) and ((sup[:, 1] > 0).sum() >= 5), which


def test_entered_maps_on_A(inputs):
    inp = inputs["A"]
    D = _entered(inp)
    per_level = [0] * inp["n_levels"]
    for (v, l), shape in inp["shapes"].items():
        m = D.level(v, l)
        assert not (m < 0).any(), (v, l)
        per_level[l] += int((m < dei.MAX_DEPTH).sum())
    print("cells below 1000 per level on A:", per_level)
    assert sum(per_level) >= 1000
    cells = [sum(c * r for (v, l), (c, r) in inp["shapes"].items() if l == lv) for lv in range(inp["n_levels"])]
    for lv in range(inp["n_levels"]):
        if cells[lv]:
            assert per_level[lv] >= 20, (lv, per_level)
    assert cells[4] > 0 and cells[5] == 0     # (no view of A has a cell on its last level)


@pytest.mark.parametrize("which", ["A", "B"])
def test_gates_over_entered_maps_vary(inputs, which):
    inp = inputs[which]
    D = _entered(inp)
    assert dei.n_written(D, inp["shapes"]) >= 1000
    idx = np.arange(inp["P"].n)
    g = dei.gates(D, inp["O"], idx, 1.0, 0)
    print(which, "blocking > 0:", int((g[:, 1] > 0).sum()), " visible > 0:", int((g[:, 0] > 0).sum()), " free > 0:",
          int((g[:, 2] > 0).sum()), " max counts:", g.max(axis=0).tolist())
    if which == "A":
        assert (g[:, 1] > 0).sum() >= 50
    for col in (0, 2):
        assert (g[:, col] == 0).sum() >= 50 and (g[:, col] > 0).sum() >= 50, (which, col)
    assert g[:, 0].max() > 64 and g[:, 2].max() > 64
    g_int = dei.gates(D, inp["O"], idx, 1.0, 1)
    g_tight = dei.gates(D, inp["O"], idx, 0.05, 0)
    print(which, "abs_int differs:", int((g_int != g).any(axis=1).sum()), " margin 0.05 differs:", int((g_tight != g).any(axis=1).sum()))
    assert (g_int != g).any(axis=1).sum() >= 50
    assert (g_tight != g).any(axis=1).sum() >= 50


@pytest.mark.parametrize("which", ["A", "B"])
def test_map_content_matters(inputs, which):
    """Two independent random fills give different counts: what a test of the footprints' reads rests on."""
    from oracle import oracle as orc
    inp = inputs[which]
    D = orc.OracleDepths(inp["osc"])
    idx = np.arange(600)
    g = []
    for seed in (101, 202):
        dei.fill_oracle(D, dei.random_fill(inp["shapes"], seed))
        g.append(dei.gates(D, inp["O"], idx))
    diff = g[0] != g[1]
    print(which, "two fills differ:", int(diff.any(axis=1).sum()), diff.sum(axis=0).tolist())
    assert diff.any(axis=1).sum() >= 100
    assert (diff.sum(axis=0) >= 50).all()


def test_level_support_reaches_every_level(inputs):
    from oracle import oracle as orc
    sup = {}
    for which in ("A", "B"):
        inp = inputs[which]
        sup[which] = np.array([[orc.level_support(inp["osc"], inp["O"][k], m) for m in range(-1, 9)] for k in range(inp["P"].n)])
        assert (sup[which] == 0).any()
    B = sup["B"]
    print("patches with support on B for min_level -1..8:", (B > 0).sum(axis=0).tolist())
    assert ((B > 0).sum(axis=0) > 0).all()
    # min_level 6 is the last one the device answers from its threshold table, 7 the first it answers with the rounded level
    assert (B[:, 7] != B[:, 8]).any() or (B[:, 6] != B[:, 7]).any()
