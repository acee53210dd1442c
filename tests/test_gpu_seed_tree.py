"""The seed octree on the GPU (hpmvs_seed_tree_batch, hpmvs_amd/csrc/kernel_seed_tree.hip): the second half of Scene::initPatches
(reference src/hpmvs/Scene.cpp:183-199).

  * the clouds of tests/test_cpu_seed_tree.py through the C ABI equal the host restatement byte for byte (which that file pins to
    the sequential DynOctTree::add); host and device pointers give the same bytes;
  * the survivors of init_patches_batch on configs[0] and on a 12-view scene: frontier.seed_tree equals tests/octree_ref.py,
    .snapshot() passes hpmvs_regularize_batch's bit-equality check of every leaf centre, .cells() + cell_start through filter_level
    equal tests/filter_ref.py on the octree_ref cells, and with set_depths every depth map equals depth_reset + set_depths_batch;
  * the three refusals return HPMVS_ERR_ARG with every output untouched."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
import seed_tree_ref as sr

pytestmark = pytest.mark.gpu
HPMVS_ERR_ARG = -2
CLOUDS = sr.clouds()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sr.HostSeedTree(tmp_path_factory.mktemp("seed_tree_host"))


def _batch(center, scale):
    from hpmvs_amd import api
    n = len(scale)
    return api.Batch(np.asarray(center, np.float32).reshape(n, 4), np.zeros((n, 4), np.float32), scale, np.zeros(n, np.int32),
                     np.full((n, 1), -1, np.int32))


def _call_host(gscene, center, scale, ok, maxlevel, set_depths=0, fill=0):
    """hpmvs_seed_tree_batch with host pointers -> (status, Result); outputs preset to `fill`."""
    from hpmvs_amd import api
    n = len(scale)
    b = _batch(center, scale)
    r = sr.Result(n)
    for k in sr.FIELDS:
        getattr(r, k)[...] = fill
    pb = b.c_struct()
    okp = None if ok is None else np.ascontiguousarray(ok, dtype=np.uint8)
    pb.ok = None if okp is None else okp.ctypes.data
    info = api.SeedTreeInfo()
    rc = api.lib().hpmvs_seed_tree_batch(gscene.h, C.byref(pb), int(maxlevel), int(set_depths), C.byref(info), r.rows.ctypes.data,
                                         r.cell_start.ctypes.data, r.cell_center.ctypes.data, r.cell_width.ctypes.data,
                                         r.cell_level.ctypes.data, r.patch_center.ctypes.data, 0, None)
    r.scale = b.scale
    r.info = np.frombuffer(bytes(info), dtype=sr.INFO_DTYPE).copy()
    return rc, r


def _call_device(gscene, center, scale, ok, maxlevel, fill=0):
    """the same call with device pointers (torch tensors)"""
    import torch
    from hpmvs_amd import api
    n = len(scale)
    dev = "cuda"
    tc = torch.from_numpy(np.ascontiguousarray(center, dtype=np.float32).reshape(n, 4)).to(dev)
    ts = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32).copy()).to(dev)
    tok = None if ok is None else torch.from_numpy(np.ascontiguousarray(ok, dtype=np.uint8)).to(dev)
    r = sr.Result(n)
    outs = {k: torch.full(getattr(r, k).shape, fill, dtype=getattr(torch, str(getattr(r, k).dtype)), device=dev) for k in sr.FIELDS}
    pb = api.PatchBatch()
    pb.n, pb.max_images = n, 1
    pb.center, pb.scale = tc.data_ptr(), ts.data_ptr()
    pb.ok = None if tok is None else tok.data_ptr()
    info = api.SeedTreeInfo()
    torch.cuda.synchronize()
    rc = api.lib().hpmvs_seed_tree_batch(gscene.h, C.byref(pb), int(maxlevel), 0, C.byref(info), *[outs[k].data_ptr() for k in sr.FIELDS],
                                         1, None)
    torch.cuda.synchronize()
    for k in sr.FIELDS:
        setattr(r, k, outs[k].cpu().numpy())
    r.scale = ts.cpu().numpy()
    r.info = np.frombuffer(bytes(info), dtype=sr.INFO_DTYPE).copy()
    return rc, r


@pytest.mark.parametrize("cloud", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_kernels_equal_the_host_restatement(gpu_scene, host, cloud):
    name, center, scale, ok, maxlevel = cloud
    rc0, want = host.tree(center, scale, ok, maxlevel)
    assert rc0 == 0
    rc, got = _call_host(gpu_scene, center, scale, ok, maxlevel, fill=77)
    assert rc == 0
    for k in ("info", "scale") + sr.FIELDS:
        assert sr.same_bits(getattr(got, k), getattr(want, k)), f"{name}: {k} differs (host pointers)"
    if len(scale) == 0:
        return   # (nothing on the device to point at)
    rc, dev = _call_device(gpu_scene, center, scale, ok, maxlevel, fill=77)
    assert rc == 0
    assert dev.bytes() == got.bytes(), f"{name}: device pointers give other bytes"


def _maps(scene, gscene):
    from hpmvs_amd import api
    return [api.depth_level(gscene, v, l) for v in range(scene.n_views) for l in range(gscene.view_levels[v])]


def _real_survivors(name, scene, gscene, n_points):
    from hpmvs_amd import api, frontier, synth
    xyz, off, img = synth.make_nvm_points(scene, n_points, start_level=2, noise=1.0)
    batch = api.init_patches_batch(gscene, xyz, off, img, start_level=2, max_images=64)
    n_ok = int(batch.ok.astype(bool).sum())
    assert n_ok > 50
    center0, scale0, ok = batch.center.copy(), batch.scale.copy(), batch.ok.copy()

    # the maps the call must leave: depth_reset + set_depths_batch of the same rows (the floored scales: setDepths follows add)
    api.depth_reset(gscene)
    api.seed_tree_batch(gscene, batch, 9, set_depths=False)
    api.set_depths_batch(gscene, batch)
    want_maps = _maps(scene, gscene)
    assert any((m < 1000).any() for m in want_maps)

    batch.scale[:] = scale0
    api.depth_reset(gscene)
    tree = frontier.seed_tree(gscene, batch, patch_init_maxlevel=9, set_depths=True)
    got_maps = _maps(scene, gscene)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got_maps, want_maps))

    # == the sequential insertion
    res = sr.Result(batch.n)
    res.info["root_center"], res.info["root_width"], res.info["scale_floor"] = tree.root_center, tree.root_width, tree.scale_floor
    res.info["n_rows"], res.info["n_leaves"] = len(tree.rows), tree.n_leaves
    res.scale = batch.scale
    L = tree.n_leaves
    res.rows[:len(tree.rows)] = tree.rows; res.cell_start[:L + 1] = tree.cell_start; res.cell_center[:L] = tree.cell_center
    res.cell_width[:L] = tree.cell_width; res.cell_level[:L] = tree.cell_level; res.patch_center[:L] = tree.patch_center
    sr.assert_equals_sequential(res, center0, scale0, ok, 9, name)
    assert len(tree.rows) == n_ok and L > 20

    # regularize accepts the snapshot: its leaf check re-derives every centre and refuses one that is not bit-equal
    first = tree.rows[tree.cell_start[:-1]]
    cells = frontier._rows(batch, first)
    fl, nn, _ = frontier.regularize_level(gscene, cells, tree.cell_width, np.arange(L), np.ones(L, np.uint8), tree.snapshot())
    assert (nn >= 0).all() and np.isfinite(fl).all()
    snap = tree.snapshot()
    assert (snap.born == -1).all() and (snap.died == api.INT32_MAX).all()

    # a coarse floor: leaves with several patches; cells() + cell_start through filter_level == filter_ref on the octree_ref cells
    batch.scale[:] = scale0
    api.depth_reset(gscene)
    coarse = frontier.seed_tree(gscene, batch, patch_init_maxlevel=2, set_depths=True)
    ref = sr.sequential(center0, scale0, ok, 2)
    ref_rows = np.array([e for leaf in ref["leaves"] for e in leaf[4]])
    ref_cs = np.cumsum([0] + [len(leaf[4]) for leaf in ref["leaves"]])
    assert (np.diff(ref_cs) >= 2).sum() >= 5
    assert coarse.rows.tolist() == ref_rows.tolist() and coarse.cell_start.tolist() == ref_cs.tolist()
    cells = coarse.cells(batch)
    F = frontier.filter_level(gscene, cells, coarse.cell_start)
    rd, rk = fr.filter_cells(batch.center[ref_rows], batch.normal[ref_rows], ref_cs)
    assert np.array_equal(F.keep, rk) and F.dist.tobytes() == rd.tobytes()
    print("seed_tree", name, {"rows": n_ok, "leaves": L, "levels": np.bincount(tree.cell_level).tolist(),
                              "coarse_leaves": coarse.n_leaves, "coarse_max_cell": int(np.diff(coarse.cell_start).max())})


def test_survivors_of_configs0(tiny_scene, gpu_scene):
    _real_survivors("configs0_3v_640x480", tiny_scene, gpu_scene, 400)


def test_survivors_of_a_12_view_scene():
    from hpmvs_amd import api, synth
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        _real_survivors("12v_640x480", scene, g, 900)
    finally:
        g.close()


def test_refusals_leave_the_outputs_untouched(tiny_scene, gpu_scene):
    from hpmvs_amd import api
    _, center, scale, _, _ = CLOUDS[0]
    center, scale = center[:200].copy(), scale[:200].copy()

    def untouched(r):
        return r.scale.tobytes() == scale.tobytes() and all((getattr(r, k) == 77).all() for k in sr.FIELDS)

    for maxlevel in (-1, 22):
        rc, r = _call_host(gpu_scene, center, scale, None, maxlevel, fill=77)
        assert rc == HPMVS_ERR_ARG and untouched(r), maxlevel
        rc, r = _call_device(gpu_scene, center, scale, None, maxlevel, fill=77)
        assert rc == HPMVS_ERR_ARG and untouched(r), maxlevel
    # a bounding box that is not finite: found on the device, refused all the same
    for bad in (np.inf, -np.inf):
        c = center.copy()
        c[17, 1] = bad
        rc, r = _call_host(gpu_scene, c, scale, None, 9, fill=77)
        assert rc == HPMVS_ERR_ARG and untouched(r), bad
        rc, r = _call_device(gpu_scene, c, scale, None, 9, fill=77)
        assert rc == HPMVS_ERR_ARG and untouched(r), bad
    c = center.copy()
    c[3, 0], c[4, 0] = 3e38, -3e38   # finite extremes whose distance is not
    rc, r = _call_host(gpu_scene, c, scale, None, 9, fill=77)
    assert rc == HPMVS_ERR_ARG and untouched(r)
    # set_depths on a scene without depth maps
    fresh = api.Scene(tiny_scene, device=0)
    try:
        rc, r = _call_host(fresh, center, scale, None, 9, set_depths=1, fill=77)
        assert rc == HPMVS_ERR_ARG and untouched(r)
        rc, r = _call_host(fresh, center, scale, None, 9, set_depths=0, fill=77)
        assert rc == 0 and int(r.info[0]["n_rows"]) == 200
    finally:
        fresh.close()
