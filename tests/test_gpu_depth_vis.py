"""Depth maps as jet-coloured images on the GPU (kernel_depth_vis.hip behind Scene.depth_image / Scene.depth_jpeg): every image
equals, byte for byte, CImg's normalize(0, 255) + map(jet_LUT256()) of tests/golden/g9_depth_vis.npz or the numpy restatement
that tests/test_cpu_depth_vis.py pins to it (float32 throughout, getFullDepth included); `range` is its m, M; the JPEG is
jpeg_encode's file of the image; the maps are only read."""
import ctypes as C
import threading

import numpy as np
import pytest

import depth_vis_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def golden():
    return ref.Golden()


@pytest.fixture(scope="module")
def scene():
    """five views whose 3 x 5 depth maps have the golden images' shapes (ref.MAP_SHAPES); the 70 x 46 one: 35x23, 17x11, 8x5"""
    from hpmvs_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    sc = api.Scene(ref.make_scene(), device=0)
    api.depth_reset(sc)
    for v, shapes in enumerate(ref.MAP_SHAPES):
        for l, shape in enumerate(shapes):
            assert api.depth_level(sc, v, l).shape == shape
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def big():
    """two 642 x 362 views: level 0's map is 321 x 181 cells, 6 x 3 workgroups, no multiple of 64 either way; filled by
    set_depths_batch from seeded patches of levels 0 and 1, plus a planted minimum in the last cell"""
    from hpmvs_amd import api, synth
    syn = ref.make_scene(sizes=[(642, 362), (642, 362)], max_level=2, seed=0xDA)
    sc = api.Scene(syn, device=0)
    api.depth_reset(sc)
    for start_level, n in ((0, 6000), (1, 2000)):
        seeds = synth.make_seeds(syn, n, start_level=start_level, seed=synth.SEED + 31 + start_level)
        batch = api.Batch.from_seeds(seeds)
        batch.ok[:] = 1
        api.set_depths_batch(sc, batch)
    m0 = api.depth_level(sc, 0, 0)
    assert m0.shape == (321, 181) and (m0 < ref.MAX_DEPTH).sum() > 1000 and (api.depth_level(sc, 0, 1) < ref.MAX_DEPTH).sum() > 100
    m0[320, 180] = 1.5
    assert m0[m0 < ref.MAX_DEPTH].min() == 1.5 and (m0 == 1.5).sum() == 1
    api.depth_set_level(sc, 0, 0, m0)
    yield sc
    sc.close()


def _levels(sc, view):
    from hpmvs_amd import api
    return [api.depth_level(sc, view, l) for l in range(sc.view_levels[view])]


def test_level_images_equal_cimg_byte_for_byte(scene, golden):
    from hpmvs_amd import api
    assert np.array_equal(api.depth_colormap(), golden.lut)
    for name in golden.names:
        v, l = golden.where(name)
        planted = np.ascontiguousarray(golden.img[name].T)   # (cols, rows): the column-major map
        api.depth_set_level(scene, v, l, planted)
        rgb, (m, M) = scene.depth_image(v, l, with_range=True)
        assert rgb.shape == golden.rgb[name].shape and np.array_equal(rgb, golden.rgb[name]), name
        _, (rm, rM) = ref.image(planted, golden.lut)
        assert m == rm and M == rM, name
        assert np.array_equal(api.depth_level(scene, v, l).view(np.uint32), planted.view(np.uint32)), name


def test_combined_image_takes_the_early_return(scene, golden):
    from hpmvs_amd import api
    api.depth_reset(scene)
    levels = ref.sparse_levels(ref.MAP_SHAPES[0], 0xC0)
    levels[1] = np.where(levels[1] == ref.MAX_DEPTH, levels[1], levels[1] - np.float32(10.0)).astype(np.float32)
    # cells that are no finite number: under empty upper cells they render as empty, under a filled one as that cell
    levels[0][3, 4], levels[0][9, 9], levels[0][21, 2], levels[0][34, 22] = np.nan, np.inf, -np.inf, np.nan
    levels[1][1, 2], levels[1][4, 4], levels[1][10, 1] = ref.MAX_DEPTH, ref.MAX_DEPTH, np.nan
    levels[2][0, 1], levels[2][2, 2], levels[2][5, 0] = ref.MAX_DEPTH, ref.MAX_DEPTH, ref.MAX_DEPTH
    levels[0][0, 0] = ref.MAX_DEPTH
    levels[1][0, 0] = levels[2][0, 0] = ref.MAX_DEPTH
    for l, m in enumerate(levels):
        api.depth_set_level(scene, 0, l, m)
    full = ref.combined(levels)
    only0 = ref.cell_depth(levels[0])
    assert np.array_equal(full[34], only0[34]) and not np.array_equal(full[:32], only0[:32])   # 34 >> 1 = 17: outside level 1
    want, (rm, rM) = ref.image(full, golden.lut)
    rgb, (m, M) = scene.depth_image(0, with_range=True)
    assert rgb.shape == (23, 35, 3) and np.array_equal(rgb, want)
    assert m == rm == 0 and M == rM
    empty = rgb[0, 0]
    for x, y in ((3, 4), (9, 9), (21, 2), (34, 22)):
        assert full[x, y] == ref.MAX_DEPTH and np.array_equal(rgb[y, x], empty), (x, y)
    # the same cells in level 0's own image, and a NaN in level 1's
    for l in (0, 1):
        want_l, rng_l = ref.image(levels[l], golden.lut)
        got_l, got_rng = scene.depth_image(0, l, with_range=True)
        assert np.array_equal(got_l, want_l) and got_rng[0] == rng_l[0] and got_rng[1] == rng_l[1]
    assert np.array_equal(scene.depth_image(0, 0)[4, 3], empty)
    # a 1 x 1 and a 1 x 13 top level, and a top level without cells (2 x 10 over 1 x 5 over 0 x 2)
    for v in (2, 3, 4):
        lv = ref.sparse_levels(ref.MAP_SHAPES[v], 0xC1 + v, fill=0.7)
        for l, m in enumerate(lv):
            api.depth_set_level(scene, v, l, m)
        assert np.array_equal(scene.depth_image(v), ref.image(ref.combined(lv), golden.lut)[0]), v


def test_map_spanning_several_workgroups_is_only_read(big, golden):
    before = _levels(big, 0)
    for level in (0, 1, None):
        src = ref.combined(before) if level is None else before[level]
        want, (rm, rM) = ref.image(src, golden.lut)
        rgb, (m, M) = big.depth_image(0, level, with_range=True)
        assert np.array_equal(rgb, want), level
        assert m == rm and M == rM, level
    assert big.depth_image(0, 0).shape == (181, 321, 3)
    _, (m, M) = big.depth_image(0, 0, with_range=True)
    assert m == 0 and M > 20                                   # the empty cells; the planted 1.5 is the least DEPTH, not m
    after = _levels(big, 0)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_planted_minimum_in_the_last_cell_is_m_when_no_cell_is_empty(big, golden):
    from hpmvs_amd import api
    keep = api.depth_level(big, 1, 0)
    rng = np.random.default_rng(0xDB)
    m1 = rng.uniform(20.0, 45.0, size=keep.shape).astype(np.float32)
    m1[320, 180], m1[0, 0] = 1.5, 46.0
    api.depth_set_level(big, 1, 0, m1)
    want, _ = ref.image(m1, golden.lut)
    rgb, (m, M) = big.depth_image(1, 0, with_range=True)
    assert np.array_equal(rgb, want) and m == np.float32(1.5) and M == np.float32(46.0)
    assert np.array_equal(rgb[180, 320], golden.lut[0]) and np.array_equal(rgb[0, 0], golden.lut[255])
    api.depth_set_level(big, 1, 0, keep)


def test_jpeg_is_the_encoders_file_of_the_image(scene, big):
    from hpmvs_amd import api
    api.depth_reset(scene)
    for v in (0, 1):
        for l, m in enumerate(ref.sparse_levels(ref.MAP_SHAPES[v], 0xE0 + v)):
            api.depth_set_level(scene, v, l, m)
    for sc, view, level in ((scene, 0, 0), (scene, 1, 0), (scene, 1, 2), (scene, 0, None), (scene, 1, None), (big, 0, None)):
        rgb = sc.depth_image(view, level)
        for q in (100, 75):
            data = sc.depth_jpeg(view, level, q)
            assert data[:2] == b"\xff\xd8" and data == api.jpeg_encode(rgb, q), (view, level, q)


def test_error_handling(scene):
    from hpmvs_amd import api
    L = api.lib()
    w, h, n = C.c_int(), C.c_int(), C.c_size_t(0)
    # depth_image: a tight buffer, and one byte short (nothing is written)
    assert L.hpmvs_scene_depth_image(scene.h, 0, 0, None, 0, 0, C.byref(w), C.byref(h), None) == ref.HPMVS_OK
    assert (w.value, h.value) == (35, 23)
    nb = 3 * 35 * 23
    raw = np.full(2 * GUARD + nb, 0xA5, np.uint8)
    assert L.hpmvs_scene_depth_image(scene.h, 0, 0, raw.ctypes.data + GUARD, nb, 0, None, None, None) == ref.HPMVS_OK
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nb:] == 0xA5).all()
    assert np.array_equal(raw[GUARD:GUARD + nb].reshape(23, 35, 3), scene.depth_image(0, 0))
    raw[:] = 0xA5
    assert L.hpmvs_scene_depth_image(scene.h, 0, 0, raw.ctypes.data + GUARD, nb - 1, 0, None, None, None) == ref.HPMVS_ERR_ARG
    assert "smaller" in L.hpmvs_last_error().decode() and (raw == 0xA5).all()
    # depth_jpeg: the bound, exactly the file's length, one byte short
    data = scene.depth_jpeg(0, 0)
    assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 0, 100, None, 0, C.byref(n)) == ref.HPMVS_OK
    assert n.value == api.jpeg_encode_bound(35, 23) >= len(data)
    raw = np.full(2 * GUARD + len(data), 0xA5, np.uint8)
    assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 0, 100, raw.ctypes.data + GUARD, len(data), C.byref(n)) == ref.HPMVS_OK
    assert n.value == len(data) and raw[GUARD:GUARD + len(data)].tobytes() == data
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + len(data):] == 0xA5).all()
    raw[:] = 0xA5
    n.value = 0
    assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 0, 100, raw.ctypes.data + GUARD, len(data) - 1, C.byref(n)) == ref.HPMVS_ERR_ARG
    assert n.value == len(data) and (raw == 0xA5).all() and "too small" in L.hpmvs_last_error().decode()
    for q in (0, 101):
        assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 0, q, raw.ctypes.data, raw.nbytes, C.byref(n)) == ref.HPMVS_ERR_ARG
    assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 0, 100, raw.ctypes.data, raw.nbytes, None) == ref.HPMVS_ERR_ARG
    # the 8 x 5 map has an image and no JPEG: the encoder's lower bound
    assert scene.depth_image(0, 2).shape == (5, 8, 3)
    for out in (None, raw.ctypes.data):
        assert L.hpmvs_scene_depth_jpeg(scene.h, 0, 2, 100, out, raw.nbytes, C.byref(n)) == ref.HPMVS_ERR_UNSUPPORTED
        assert "8 pixels" in L.hpmvs_last_error().decode()
    # a map without cells: an empty image
    assert scene.depth_image(4, 2).shape == (2, 0, 3)
    # a bad view / level: the depth-map entries' code and message
    for view, level in ((-1, 0), (5, 0), (0, 3), (0, -2), (0, 8)):
        assert L.hpmvs_scene_depth_image(scene.h, view, level, None, 0, 0, C.byref(w), C.byref(h), None) == ref.HPMVS_ERR_ARG
        assert "scene_depth_image: bad view / level" in L.hpmvs_last_error().decode()
        assert L.hpmvs_scene_depth_jpeg(scene.h, view, level, 100, None, 0, C.byref(n)) == ref.HPMVS_ERR_ARG
        assert "scene_depth_jpeg: bad view / level" in L.hpmvs_last_error().decode()
    assert L.hpmvs_scene_depth_get_level(scene.h, 0, 3, None, 0, None, None) == ref.HPMVS_ERR_ARG   # (the existing entry's)
    # no depth maps yet
    fresh = api.Scene(ref.make_scene(sizes=[(70, 46)]), device=0)
    try:
        assert L.hpmvs_scene_depth_image(fresh.h, 0, 0, None, 0, 0, C.byref(w), C.byref(h), None) == ref.HPMVS_ERR_STATE
        assert "scene_depth_image: call hpmvs_scene_depth_reset first" in L.hpmvs_last_error().decode()
        assert L.hpmvs_scene_depth_jpeg(fresh.h, 0, ref.COMBINED, 100, None, 0, C.byref(n)) == ref.HPMVS_ERR_STATE
        with pytest.raises(api.HpmvsError):
            fresh.depth_image(0)
        with pytest.raises(api.HpmvsError):
            fresh.depth_jpeg(0, 0)
    finally:
        fresh.close()


def test_image_into_device_memory(scene):
    import torch
    from hpmvs_amd import api
    want = scene.depth_image(1, None)
    out = torch.zeros(want.shape, dtype=torch.uint8, device="cuda:0")
    rng = (C.c_float * 2)()
    api._chk(api.lib().hpmvs_scene_depth_image(scene.h, 1, ref.COMBINED, out.data_ptr(), out.numel(), 1, None, None, rng))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert (rng[0], rng[1]) == tuple(scene.depth_image(1, None, with_range=True)[1])


def test_two_threads_render_different_views_at_once(big):
    single = [(big.depth_image(v, None), big.depth_jpeg(v, 0, 75)) for v in (0, 1)]
    got = [[], []]
    errors = []

    def work(v):
        try:
            for _ in range(4):
                got[v].append((big.depth_image(v, None), big.depth_jpeg(v, 0, 75)))
        except Exception as e:   # (reported below: an exception in a thread fails nothing by itself)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(v,)) for v in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for v in (0, 1):
        assert len(got[v]) == 4
        for rgb, jpg in got[v]:
            assert np.array_equal(rgb, single[v][0]) and jpg == single[v][1]
