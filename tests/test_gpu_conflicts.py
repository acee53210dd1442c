"""The conflict graph of an extend level on the device (hpmvs_conflicts_from_footprints, hpmvs_level_conflicts_batch; DESIGN.md
§3.18) against the definition by set intersection in Python (tests/conflicts_ref.py), byte for byte: the hand-written and the
random synthetic footprints of tests/test_cpu_conflicts.py with host and with device pointers, n == 0, the capacity contract,
every refusal with poisoned outputs, and the refined candidates of one extend level of two real scenes, without and with the
filter's losers as events."""
import ctypes as C

import numpy as np
import pytest

import conflicts_ref as cr

pytestmark = pytest.mark.gpu
HPMVS_ERR_ARG, HPMVS_ERR_STATE = -2, -3
POISON = 0xABABABAB


@pytest.fixture(scope="module")
def references():
    """Every synthetic case with the definition's graph, computed once."""
    cases = [(c[0],) + tuple(c[1:8]) for c in cr.known_answers()]
    cases += [("random n%d V%d L%d M%d ev%d" % c[1:6],) + cr.random_case(c) for c in cr.RANDOM_CASES]
    return [(name, ni, wr, fr, at, vb, ev, L, cr.graph_bytes(cr.definition(ni, wr, fr, at, vb, L, ev))) for name, ni, wr, fr, at, vb, ev, L in cases]


def test_synthetic_footprints_with_host_pointers(references):
    from hpmvs_amd import api
    assert api.device_count() >= 1
    for name, ni, wr, fr, at, vb, ev, L, want in references:
        got = api.conflicts_from_footprints(ni, wr, fr, at, vb, L, ev)
        assert cr.graph_bytes(got) == want, name


def _raw(n, M, V, L, ni, wr, fr, at, vb, ev, fo, fa, cf, ao, aa, ca, on_device=0):
    """hpmvs_conflicts_from_footprints as it is: pointers as integers (None: null); -> (status, n_flow, n_anti, error text)"""
    from hpmvs_amd import api
    nf, na = C.c_uint32(POISON), C.c_uint32(POISON)
    rc = api.lib().hpmvs_conflicts_from_footprints(0, n, M, V, L, ni, wr, fr, at, vb, ev, fo, fa, cf, ao, aa, ca, C.byref(nf), C.byref(na), on_device, None)
    return rc, nf.value, na.value, api.lib().hpmvs_last_error().decode()


def test_synthetic_footprints_with_device_pointers(references):
    import torch
    dev = torch.device("cuda:0")
    for name, ni, wr, fr, at, vb, ev, L, want in references:
        n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ni, wr, fr, at, vb)]
        tev = None if ev is None else torch.from_numpy(ev).to(dev)
        n_flow, n_anti = len(want[1]) // 4, len(want[3]) // 4
        fo = torch.full((n + 1,), 7, dtype=torch.int32, device=dev); ao = torch.full((n + 1,), 7, dtype=torch.int32, device=dev)
        fa = torch.full((n_flow + 1,), -1, dtype=torch.int32, device=dev); aa = torch.full((n_anti + 1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc, nf, na, err = _raw(n, M, V, L, *[x.data_ptr() for x in t], None if tev is None else tev.data_ptr(), fo.data_ptr(), fa.data_ptr(),
                               n_flow, ao.data_ptr(), aa.data_ptr(), n_anti, on_device=1)
        torch.cuda.synchronize()
        assert rc == 0 and (nf, na) == (n_flow, n_anti), (name, rc, err)
        got = tuple(x.cpu().numpy().view(np.uint32) for x in (fo, fa[:n_flow], ao, aa[:n_anti]))
        assert cr.graph_bytes(got) == want, name
        assert int(fa[n_flow]) == -1 and int(aa[n_anti]) == -1, name   # nothing past the lists


def test_no_nodes_is_the_empty_graph():
    from hpmvs_amd import api
    ni, wr, fr, at, vb = cr.empty_footprints(0, 3, 2)
    fo, fa, ao, aa = api.conflicts_from_footprints(ni, wr, fr, at, vb, 4)
    assert fo.tolist() == [0] and ao.tolist() == [0] and len(fa) == 0 and len(aa) == 0
    fo, ao = np.full(1, POISON, np.uint32), np.full(1, POISON, np.uint32)
    rc, nf, na, err = _raw(0, 3, 2, 4, None, None, None, None, None, None, fo.ctypes.data, None, 0, ao.ctypes.data, None, 0)
    assert rc == 0 and (nf, na) == (0, 0) and fo[0] == 0 and ao[0] == 0, err


def test_capacity_contract_too_small_then_exact(references):
    name, ni, wr, fr, at, vb, ev, L, want = next(r for r in references if r[0].startswith("random n700 V3"))
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    n_flow, n_anti = len(want[1]) // 4, len(want[3]) // 4
    assert n_flow > 1 and n_anti > 1
    ptr = [np.ascontiguousarray(a).ctypes.data for a in (ni, wr, fr, at, vb, ev)]
    for cf, ca in ((n_flow - 1, n_anti), (n_flow, n_anti - 1), (0, 0)):
        fo, ao = np.full(n + 1, POISON, np.uint32), np.full(n + 1, POISON, np.uint32)
        fa, aa = np.full(n_flow, POISON, np.uint32), np.full(n_anti, POISON, np.uint32)
        rc, nf, na, err = _raw(n, M, V, L, *ptr, fo.ctypes.data, fa.ctypes.data, cf, ao.ctypes.data, aa.ctypes.data, ca)
        assert rc == HPMVS_ERR_ARG and "capacity" in err, (rc, err)
        assert (nf, na) == (n_flow, n_anti) and fo.tobytes() == want[0] and ao.tobytes() == want[2]   # totals and offsets: always
        assert (fa == POISON).all() and (aa == POISON).all()                                          # adjacency: not at all
    rc, nf, na, err = _raw(n, M, V, L, *ptr, fo.ctypes.data, fa.ctypes.data, n_flow, ao.ctypes.data, aa.ctypes.data, n_anti)
    assert rc == 0, err
    assert cr.graph_bytes((fo, fa, ao, aa)) == want


def test_refusals_leave_poisoned_outputs_untouched():
    ni, wr, fr, at, vb, ev, L = cr.random_case((4, 65, 3, 4, 7, 3, 24))
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    fo, ao = np.full(n + 1, POISON, np.uint32), np.full(n + 1, POISON, np.uint32)
    fa, aa = np.full(4096, POISON, np.uint32), np.full(4096, POISON, np.uint32)
    p = dict(n=n, M=M, V=V, L=L, ni=ni.ctypes.data, wr=wr.ctypes.data, fr=fr.ctypes.data, at=at.ctypes.data, vb=vb.ctypes.data, ev=ev.ctypes.data,
             fo=fo.ctypes.data, fa=fa.ctypes.data, cf=fa.size, ao=ao.ctypes.data, aa=aa.ctypes.data, ca=aa.size)
    bad = [dict(L=0), dict(L=9), dict(M=0), dict(M=257), dict(V=0), dict(n=-1), dict(ni=None), dict(wr=None), dict(fr=None), dict(at=None),
           dict(vb=None), dict(fo=None), dict(ao=None), dict(fa=None), dict(aa=None)]
    for change in bad:
        rc, nf, na, err = _raw(**{**p, **change})
        assert rc == HPMVS_ERR_ARG and (nf, na) == (POISON, POISON), (change, rc, err)
        assert all((a == POISON).all() for a in (fo, ao, fa, aa)), change
    # every node on one cell: more than 2^30 (reader, writer) pairs before duplicates are dropped
    n, M = 3072, 8
    ni, wr, fr, at, vb = cr.empty_footprints(n, M, 1)
    ni[:] = M; wr[:] = (0, 0, 1, 1); fr[:] = (0, 0, 1, 1); at[:] = (0, 2, 2)
    fo, ao = np.full(n + 1, POISON, np.uint32), np.full(n + 1, POISON, np.uint32)
    rc, nf, na, err = _raw(n, M, 1, 1, ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data, vb.ctypes.data, None, fo.ctypes.data,
                           fa.ctypes.data, fa.size, ao.ctypes.data, aa.ctypes.data, aa.size)
    assert rc == HPMVS_ERR_STATE and (nf, na) == (POISON, POISON), (rc, err)
    assert all((a == POISON).all() for a in (fo, ao, fa, aa))


# ---- real scenes: the nodes of one extend level (init-patch survivors grouped into the grid cells of a wide leaf, filtered; the
# kept patches' refined candidates, and in the second case every cell's losers before them as events)
def _level_nodes(scene, gscene, n_seeds, seed_off):
    from hpmvs_amd import api, frontier, synth
    seeds = synth.make_seeds(scene, n_seeds, start_level=2, seed=synth.SEED + seed_off)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gscene, b)
    k = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
    width = float(np.float32(3.0 * 2.0 * np.median(R.scale) / 0.9))
    cells = {}
    for i in range(R.n):
        cells.setdefault(frontier.cell_key(R.center[i], width), []).append(i)
    idx = [i for rows in cells.values() for i in rows]
    cs = np.concatenate([[0], np.cumsum([len(rows) for rows in cells.values()])]).astype(np.int32)
    P = frontier._rows(R, idx)
    api.depth_reset(gscene)
    P.ok[:] = 1
    api.set_depths_batch(gscene, P)
    F = frontier._filter(gscene, P, cs)
    parents = frontier._rows(P, F.keep)
    # (no leaf counts as occupied: every candidate is refined, so that the level has a few hundred nodes)
    out, _, _, skip, refined, _ = frontier._candidates(gscene, parents, width, frontier._GridKeys(frontier.cell_key, width, set()),
                                                       api.default_options())
    M = max(out.max_images, P.max_images)
    cands = frontier._rows(out, np.nonzero(refined)[0], M)
    # with events: per cell its losers, then its refined candidates
    rows, is_ev = [], []
    both = frontier._concat([frontier._rows(out, np.arange(out.n), M), frontier._rows(P, np.arange(P.n), M)])
    for c in range(len(cs) - 1):
        for r in range(int(cs[c]), int(cs[c + 1])):
            if F.removed[r]:
                rows.append(out.n + r); is_ev.append(1)
        for t in range(6 * c, 6 * c + 6):
            if refined[t]:
                rows.append(t); is_ev.append(0)
    return cands, frontier._rows(both, rows), np.array(is_ev, np.uint8)


def _check_level(gscene, nodes, is_ev, what):
    from hpmvs_amd import api, frontier
    wr, fr, at, vb = api.depth_footprints_batch(gscene, nodes)
    want = cr.definition(nodes.n_images, wr, fr, at, vb, frontier._pyramid_levels(gscene, what), is_ev)
    got = api.level_conflicts(gscene, nodes, is_ev)
    assert cr.graph_bytes(got) == cr.graph_bytes(want), what
    assert len(want[1]) + len(want[3]) > 0, (what, "the level has no conflicts: the scene checks nothing")
    return want


def test_level_conflicts_on_configs0(tiny_scene, gpu_scene):
    cands, nodes, is_ev = _level_nodes(tiny_scene, gpu_scene, 400, 11)
    assert cands.n >= 100
    _check_level(gpu_scene, cands, None, "configs0 candidates")
    assert is_ev.sum() >= 10
    want = _check_level(gpu_scene, nodes, is_ev, "configs0 with events")
    ev = np.nonzero(is_ev)[0]
    assert sum(int(want[0][i + 1] - want[0][i]) + int(want[2][i + 1] - want[2][i]) for i in ev) > 0   # the events take part


def test_level_conflicts_on_a_12_view_scene():
    from hpmvs_amd import api, synth
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        cands, nodes, is_ev = _level_nodes(scene, g, 500, 0)
        assert cands.n >= 100
        _check_level(g, cands, None, "12 views candidates")
        assert is_ev.sum() >= 5
        _check_level(g, nodes, is_ev, "12 views with events")
    finally:
        g.close()
