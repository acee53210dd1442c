"""CellProcessor::filter (reference src/hpmvs/CellProcessor.cpp:43-82) on the GPU, and processCell's first visit of a level whose leaves
hold several patches (:377-392: filter, then extend the kept patch), against the float32 restatement (tests/filter_ref.py) and the
oracle's sequential loop: per cell in queue order the restated filter, the losers' orc_set_depths_ex(..., 1), then orc_extend_round on
the kept patch (counts from the live maps).

  * hpmvs_filter_batch: dist bit for bit and keep equal on random cells of 1 .. 5000 patches (ties, zero normals, NaN / inf centres,
    a cell without winner); host and device pointers give the same bytes; malformed offsets are refused with outputs untouched.
  * frontier.filter_level: every depth map equals the oracle's call-by-call subtraction loop.
  * frontier.filter_extend_level: keep, dist, stage codes, counts, accepted set, occupancy, refined candidates and every depth map
    equal the sequential loop on configs[0] and on a 12-view scene; "all filters first, then extend" gives a different result;
    a cell of a few hundred patches does not multiply the waves.
  * On single-patch levels filter_extend_level is extend_level, wave for wave."""
import ctypes as C
import json

import numpy as np
import pytest

import filter_ref as fr

pytestmark = pytest.mark.gpu
MARGIN = 1.0


def _record(name, rec):
    print(name, json.dumps(rec))


def _same_dist(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].view(np.uint32).tobytes() == b[~nb].view(np.uint32).tobytes()


def _random_cells(rng):
    sizes = list(rng.integers(2, 11, size=600)) + [1] * 80 + [0] * 20 + list(rng.integers(11, 200, size=30)) + [1000, 5000, 2500]
    sizes = [int(s) for s in rng.permutation(sizes)]
    n = sum(sizes)
    cen = np.ones((n, 4), np.float32)
    nor = np.zeros((n, 4), np.float32)
    cen[:, :3] = rng.normal(0, 1, (n, 3)).astype(np.float32) * np.float32(3.0)
    nor[:, :3] = rng.normal(0, 1, (n, 3)).astype(np.float32) * rng.choice([1e-3, 1.0, 50.0], size=(n, 1)).astype(np.float32)
    cs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    special = []
    for c in range(len(sizes)):
        s, e = int(cs[c]), int(cs[c + 1])
        if e - s < 3 or len(special) >= 60:
            continue
        kind = len(special) % 6
        if kind == 0:    # exact ties: the same patch twice, a plane through both
            cen[s + 1] = cen[s]; nor[s + 1] = nor[s]
            cen[s:e, :3] = np.round(cen[s:e, :3]); nor[s:e, :3] = np.float32([0, 0, 1])
        elif kind == 1:  # zero normals
            nor[s, :3] = 0
        elif kind == 2:  # a NaN centre: no winner in the cell
            cen[s + 1, 2] = np.nan
        elif kind == 3:  # an inf centre
            cen[s, 0] = np.inf
        elif kind == 4:  # every row tied at 0
            cen[s:e, :3] = cen[s, :3]
        else:            # -inf / +inf mixes
            cen[s + 1, 1] = -np.inf
        special.append((c, kind))
    return cen, nor, cs


def _batch(cen, nor):
    from hpmvs_amd import api
    n = len(cen)
    return api.Batch(cen, nor, np.ones(n, np.float32), np.ones(n, np.int32), np.zeros((n, 1), np.int32))


def test_filter_kernel_equals_the_restatement(gpu_scene):
    import torch
    from hpmvs_amd import api
    rng = np.random.default_rng(5)
    cen, nor, cs = _random_cells(rng)
    b = _batch(cen, nor)
    dist, keep = api.filter_batch(gpu_scene, b, cs)
    rd, rk = fr.filter_cells(cen, nor, cs)
    assert _same_dist(dist, rd), np.nonzero(dist.view(np.uint32) != rd.view(np.uint32))[0][:10]
    assert np.array_equal(keep, rk), np.nonzero(keep != rk)[0][:10]
    sizes = np.diff(cs)
    assert (rk == -2).sum() >= 5 and (rk == -1).sum() == 20 and sizes.max() == 5000
    # a tie that is decided by the index, not by the value
    ties = sum(1 for c in range(len(sizes)) if rk[c] >= 0 and (rd[cs[c]:cs[c + 1]] == rd[rk[c]]).sum() > 1)
    assert ties >= 10
    # device pointers: the same bytes
    dev = "cuda"
    tc, tn = torch.from_numpy(cen).to(dev), torch.from_numpy(nor).to(dev)
    tcs = torch.from_numpy(cs).to(dev)
    td = torch.full((len(cen),), 7.0, dtype=torch.float32, device=dev)
    tk = torch.full((len(cs) - 1,), 99, dtype=torch.int32, device=dev)
    pb = api.PatchBatch()
    pb.n, pb.max_images = len(cen), 1
    pb.center, pb.normal = tc.data_ptr(), tn.data_ptr()
    rc = api.lib().hpmvs_filter_batch(gpu_scene.h, C.byref(pb), tcs.data_ptr(), len(cs) - 1, td.data_ptr(), tk.data_ptr(), 1, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert td.cpu().numpy().tobytes() == dist.tobytes() and np.array_equal(tk.cpu().numpy(), keep)
    # malformed offsets: HPMVS_ERR_ARG, outputs untouched, host and device pointers
    for bad in ([1], [0, 3, 2, 5], [0, 2, 3], [0, 2, 9]):
        bcs = np.array(bad, np.int32)
        n = 5
        bb = _batch(cen[:n], nor[:n])
        d = np.full(n, 7.0, np.float32); k = np.full(len(bcs) - 1, 99, np.int32)
        rc = api.lib().hpmvs_filter_batch(gpu_scene.h, C.byref(bb.c_struct()), bcs.ctypes.data, len(bcs) - 1, d.ctypes.data, k.ctypes.data, 0, None)
        assert rc == -2 and (d == 7.0).all() and (k == 99).all(), bad
        tb = torch.from_numpy(bcs).to(dev)
        td = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        tk = torch.full((max(1, len(bcs) - 1),), 99, dtype=torch.int32, device=dev)
        pb = api.PatchBatch()
        pb.n, pb.max_images = n, 1
        pb.center, pb.normal = tc.data_ptr(), tn.data_ptr()
        rc = api.lib().hpmvs_filter_batch(gpu_scene.h, C.byref(pb), tb.data_ptr(), len(bcs) - 1, td.data_ptr(), tk.data_ptr(), 1, None)
        torch.cuda.synchronize()
        assert rc == -2 and (td.cpu().numpy() == 7.0).all() and (tk.cpu().numpy() == 99).all(), bad
    rc = api.lib().hpmvs_filter_batch(gpu_scene.h, C.byref(b.c_struct()), cs.ctypes.data, -1, None, None, 0, None)
    assert rc == -2
    hist = np.bincount(np.minimum(sizes, 11))
    _record("filter_kernel", {"cells": int(len(sizes)), "rows": int(cs[-1]), "no_winner": int((rk == -2).sum()),
                              "index_ties": int(ties), "size_hist_0_to_10_and_more": hist.tolist()})


# ---- levels on real scenes: init-patch survivors grouped into the grid cells of a wide leaf
def _survivors(scene, gscene, n_seeds, seed_off):
    from hpmvs_amd import api, synth
    seeds = synth.make_seeds(scene, n_seeds, start_level=2, seed=synth.SEED + seed_off)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gscene, b)
    k = np.nonzero(b.ok)[0]
    return api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])


def _grid_cells(R, width, extra=None):
    """Rows grouped by leaf (cells in first-appearance order, rows in survivor order); extra[(cell, rows)] appends more rows."""
    from hpmvs_amd import api, frontier
    keys = [frontier.cell_key(R.center[i], width) for i in range(R.n)]
    order, first = [], {}
    for i, k in enumerate(keys):
        if k not in first:
            first[k] = len(order)
            order.append([])
        order[first[k]].append(i)
    idx = [i for cell in order for i in cell]
    cs = np.concatenate([[0], np.cumsum([len(c) for c in order])]).astype(np.int32)
    P = api.Batch(R.center[idx], R.normal[idx], R.scale[idx], R.n_images[idx], R.images[idx])
    return P, cs, set(first)


def _enter_all(gscene, OD, P):
    from hpmvs_amd import api
    api.depth_reset(gscene)
    P.ok[:] = 1
    api.set_depths_batch(gscene, P)
    if OD is not None:
        for i in range(P.n):
            OD.set_depths(fr.oracle_patch(P, i)[0])


def _maps_equal(gscene, OD):
    from hpmvs_amd import api
    for v in range(gscene.n_views):
        for l in range(gscene.view_levels[v]):
            a, b = api.depth_level(gscene, v, l), OD.level(v, l)
            if not np.array_equal(a, b):
                return False, (v, l, int((a != b).sum()))
    return True, None


def _width(R, factor):
    return float(np.float32(factor * 2.0 * np.median(R.scale) / 0.9))


def test_filter_level_maps_equal_the_subtraction_loop(tiny_scene, gpu_scene, oracle_scene):
    from hpmvs_amd import frontier
    from oracle import oracle as orc
    R = _survivors(tiny_scene, gpu_scene, 400, 11)
    P, cs, _ = _grid_cells(R, _width(R, 3.0))
    OD = orc.OracleDepths(oracle_scene)
    _enter_all(gpu_scene, OD, P)
    res = frontier.filter_level(gpu_scene, P, cs)
    rd, rk = fr.filter_cells(P.center, P.normal, cs)
    assert _same_dist(res.dist, rd) and np.array_equal(res.keep, rk)
    for c in range(len(cs) - 1):
        for r in range(int(cs[c]), int(cs[c + 1])):
            if r != rk[c]:
                OD.set_depths(fr.oracle_patch(P, r)[0], subtract=True)
    ok, where = _maps_equal(gpu_scene, OD)
    assert ok, where
    assert int(res.removed.sum()) >= 20 and res.removed.sum() == P.n - (len(cs) - 1)
    _record("filter_level", {"rows": P.n, "cells": len(cs) - 1, "losers": int(res.removed.sum())})


def _compare_sequential(tag, scene, gscene, oscene, P, cs, occ0, width, abs_int=0):
    """filter_extend_level vs the sequential loop from the same maps; returns (record, oracle candidates, counts, maps-equal-to)."""
    from hpmvs_amd import frontier
    from oracle import oracle as orc
    OD = orc.OracleDepths(oscene)
    _enter_all(gscene, OD, P)
    occ_g, occ_c = set(occ0), set(occ0)
    F, L = frontier.filter_extend_level(gscene, P, cs, width, occ_g, margin=MARGIN, abs_int=abs_int)
    dist, keep, cand, cnt = fr.sequential_filter_extend(oscene, OD, P, cs, width, occ_c, MARGIN, abs_int)
    n = len(cs) - 1
    st = np.array([cand[t].stage for t in range(6 * n)])
    assert np.array_equal(F.keep, keep) and _same_dist(F.dist, dist), tag
    diff = np.nonzero(L.stage != st)[0]
    assert len(diff) == 0, (tag, diff[:10], L.stage[diff[:10]], st[diff[:10]])
    assert np.array_equal(L.counts, cnt), (tag, np.nonzero((L.counts != cnt).any(axis=1))[0][:10])
    for t in range(6 * n):
        if st[t] in (0, 21, 22, 23, 24, 25, 26):
            assert np.array_equal(np.array(cand[t].center[:], dtype=np.float32), L.candidates.center[t]), (tag, t)
            assert np.array_equal(np.array(cand[t].normal[:], dtype=np.float32), L.candidates.normal[t]), (tag, t)
    assert occ_g == occ_c, tag
    ok, where = _maps_equal(gscene, OD)
    assert ok, (tag, where)
    assert L.accepted == [t for t in range(6 * n) if st[t] == 0], tag
    rec = {"scene": tag, "rows": P.n, "cells": n, "losers": int(F.removed.sum()), "largest_cell": int(np.diff(cs).max()),
           "accepted": len(L.accepted), "waves": L.waves, "deferred_per_wave": L.deferred_per_wave}
    return rec, OD, st, cnt


def _filters_first(gscene, oscene, P, cs, occ0, width, keep):
    """The wrong order, on the oracle: every loser out first, then extend over all kept patches."""
    from oracle import oracle as orc
    OD = orc.OracleDepths(oscene)
    _enter_all(gscene, OD, P)
    kept = set(keep.tolist())
    for r in range(P.n):
        if r not in kept:
            OD.set_depths(fr.oracle_patch(P, r)[0], subtract=True)
    par = (orc.Patch * len(keep))(*[fr.oracle_patch(P, int(k))[0] for k in keep])
    occ = set(occ0)
    cand, cnt = orc.extend_round(oscene, OD, par, width, occ, MARGIN, 0, frozen_gates=False)
    return OD, np.array([cand[t].stage for t in range(6 * len(keep))]), cnt


def _differs(gscene, OD_a, OD_b, st_a, st_b, cnt_a, cnt_b):
    if not np.array_equal(st_a, st_b) or not np.array_equal(cnt_a, cnt_b):
        return True
    return any(not np.array_equal(OD_a.level(v, l), OD_b.level(v, l)) for v in range(gscene.n_views) for l in range(gscene.view_levels[v]))


def _single_patch(P, cs, keep):
    from hpmvs_amd import api
    k = np.asarray(keep)
    return api.Batch(P.center[k], P.normal[k], P.scale[k], P.n_images[k], P.images[k])


def _level_checks(tag, scene, gscene, oscene, R, factor):
    from hpmvs_amd import api, frontier
    width = _width(R, factor)
    P, cs, occ0 = _grid_cells(R, width)
    assert P.n - (len(cs) - 1) >= 10, (tag, "too few multi-patch leaves")
    rec, OD, st, cnt = _compare_sequential(tag, scene, gscene, oscene, P, cs, occ0, width)
    rec["width"] = width
    ODf, stf, cntf = _filters_first(gscene, oscene, P, cs, occ0, width, np.asarray([int(x) for x in fr.filter_cells(P.center, P.normal, cs)[1]]))
    rec["filters_first_differs"] = bool(_differs(gscene, OD, ODf, st, stf, cnt, cntf))
    # the same leaves reduced to their kept patch: extend_level's waves
    keep = fr.filter_cells(P.center, P.normal, cs)[1]
    S = _single_patch(P, cs, keep)
    api.depth_reset(gscene)
    S.ok[:] = 1
    api.set_depths_batch(gscene, S)
    rec["single_patch_waves"] = frontier.extend_level(gscene, S, width, set(occ0), MARGIN, 0).waves
    return rec, P, cs, occ0, width


def _big_cell(R, P, cs, occ0, width, m, rng):
    """Cell 0 gets m - 1 more patches: jittered copies of its first patch that stay in its leaf (seeds refining to one point)."""
    from hpmvs_amd import api, frontier
    k0 = frontier.cell_key(P.center[0], width)
    rows = []
    while len(rows) < m - 1:
        c = P.center[0].copy()
        c[:3] += (rng.normal(0, 0.15, 3) * width).astype(np.float32)
        if frontier.cell_key(c, width) == k0:
            rows.append(c)
    e = int(cs[1])
    ins = np.array(rows, np.float32)
    rep = lambda a: np.repeat(a[:1], m - 1, axis=0)
    B = api.Batch(np.concatenate([P.center[:e], ins, P.center[e:]]), np.concatenate([P.normal[:e], rep(P.normal), P.normal[e:]]),
                  np.concatenate([P.scale[:e], rep(P.scale), P.scale[e:]]), np.concatenate([P.n_images[:e], rep(P.n_images), P.n_images[e:]]),
                  np.concatenate([P.images[:e], rep(P.images), P.images[e:]]))
    cs2 = cs.copy()
    cs2[1:] += m - 1
    return B, cs2


def test_filter_extend_level_equals_the_sequential_loop_on_configs0(tiny_scene, gpu_scene, oracle_scene):
    R = _survivors(tiny_scene, gpu_scene, 400, 11)
    rec, P, cs, occ0, width = _level_checks("configs0_3v_640x480", tiny_scene, gpu_scene, oracle_scene, R, 3.0)
    # a level whose first leaf holds a few hundred patches: equal to the sequential loop, and the waves do not grow with it
    B, cs2 = _big_cell(R, P, cs, occ0, width, 300, np.random.default_rng(3))
    big, _, _, _ = _compare_sequential("configs0_big_cell", tiny_scene, gpu_scene, oracle_scene, B, cs2, occ0, width)
    assert big["largest_cell"] >= 300
    assert big["waves"] <= max(2 * rec["single_patch_waves"], rec["single_patch_waves"] + 3), (big, rec)
    _record("filter_extend_level", rec)
    _record("filter_extend_level_big_cell", {**big, "single_patch_waves": rec["single_patch_waves"]})


def test_filter_extend_level_equals_the_sequential_loop_on_a_12_view_scene():
    from hpmvs_amd import api, synth
    from oracle import oracle as orc
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        R = _survivors(scene, g, 900, 0)
        rec, *_ = _level_checks("12v_640x480", scene, g, orc.OracleScene(scene), R, 3.0)
    finally:
        g.close()
    _record("filter_extend_level", rec)
    # the interleaving is part of the result: on this scene "every filter first, then extend" differs from the sequential loop
    assert rec["filters_first_differs"], rec


@pytest.mark.parametrize("abs_int", [0, 1])
def test_single_patch_levels_are_extend_level(abs_int, tiny_scene, gpu_scene):
    from hpmvs_amd import api, frontier
    R = _survivors(tiny_scene, gpu_scene, 200, 0)
    width = _width(R, 1.0)
    P, cs, occ0 = _grid_cells(R, width)
    keep = cs[:-1]
    S = _single_patch(P, cs, keep)   # the first patch of every leaf: one patch per cell
    out = {}
    for mode in ("extend", "filter_extend"):
        api.depth_reset(gpu_scene)
        S.ok[:] = 1
        api.set_depths_batch(gpu_scene, S)
        occ = set(occ0)
        if mode == "extend":
            L = frontier.extend_level(gpu_scene, S, width, occ, MARGIN, abs_int)
        else:
            F, L = frontier.filter_extend_level(gpu_scene, S, np.arange(S.n + 1), width, occ, margin=MARGIN, abs_int=abs_int)
            assert F.removed.sum() == 0 and np.array_equal(F.keep, np.arange(S.n)) and not F.dist.any()
        maps = [api.depth_level(gpu_scene, v, l).tobytes() for v in range(gpu_scene.n_views) for l in range(gpu_scene.view_levels[v])]
        out[mode] = (L, occ, maps)
    a, b = out["extend"], out["filter_extend"]
    assert np.array_equal(a[0].stage, b[0].stage) and np.array_equal(a[0].counts, b[0].counts)
    assert a[0].accepted == b[0].accepted and a[0].waves == b[0].waves and a[0].deferred_per_wave == b[0].deferred_per_wave
    assert a[0].candidates.center.tobytes() == b[0].candidates.center.tobytes()
    assert a[1] == b[1] and a[2] == b[2]
    assert len(a[0].accepted) >= 5


def test_filter_extend_level_refuses_before_touching_the_maps(tiny_scene, gpu_scene):
    from hpmvs_amd import api, frontier
    R = _survivors(tiny_scene, gpu_scene, 100, 0)
    P = api.Batch(R.center[:6], R.normal[:6], R.scale[:6], R.n_images[:6], R.images[:6])
    _enter_all(gpu_scene, None, P)
    before = [api.depth_level(gpu_scene, v, 0).tobytes() for v in range(gpu_scene.n_views)]
    bad_c = P.center.copy()
    bad_c[2, 2] = np.nan
    Q = api.Batch(bad_c, P.normal, P.scale, P.n_images, P.images)
    cases = [(P, [0, 3, 3, 6], None), (Q, [0, 3, 6], None), (P, [0, 3, 6], np.ones(6, np.uint8))]
    for B, cs, exp in cases:
        with pytest.raises(ValueError):
            frontier.filter_extend_level(gpu_scene, B, cs, 1.0, set(), expanded=exp)
    with pytest.raises(ValueError):
        frontier.filter_level(gpu_scene, Q, [0, 3, 6])
    assert before == [api.depth_level(gpu_scene, v, 0).tobytes() for v in range(gpu_scene.n_views)]
