"""Depth maps as jet-coloured images, host side: the numpy restatement and the host compile of hpmvs_amd/csrc/depth_vis.hpp (the
functions kernel_depth_vis.hip calls) both give CImg's normalize(0, 255) + map(jet_LUT256()) of tests/golden/g9_depth_vis.npz
byte for byte, the colormap equals its 768 values, the two agree on getFullDepth over odd-sized levels, and the C ABI checks
its arguments before it looks for a device."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_vis_ref as ref

CASES = ["all_empty", "one_depth", "one_cell", "min_first_max_last", "max_first_min_last", "negative", "range_0_255",
         "on_and_below_integers", "sparse_64x48", "dense_35x23", "one_by_one", "one_by_n", "sparse_5x4"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ref.HostDepthVis(tmp_path_factory.mktemp("depth_vis_host"))


@pytest.fixture(scope="module")
def golden():
    return ref.Golden()


def test_fixture_is_what_the_issue_lists(golden):
    assert os.path.getsize(ref.GOLDEN) < 64 * 1024
    assert golden.names == CASES and golden.lut.shape == (256, 3) and golden.lut.dtype == np.uint8
    for n in CASES:
        h, w = golden.img[n].shape
        assert w <= 64 and h <= 48 and golden.rgb[n].shape == (h, w, 3) and np.isfinite(golden.img[n]).all()
        golden.where(n)   # (the GPU test's scene has a map of this shape)
    img = golden.img
    assert (img["all_empty"] == ref.MAX_DEPTH).all()
    assert len(np.unique(img["one_depth"])) == 1 and (img["one_depth"] != ref.MAX_DEPTH).all()
    assert (img["one_cell"] != ref.MAX_DEPTH).sum() == 1
    a = ref.cell_value(img["min_first_max_last"])
    assert a.flat[0] == a.min() and a.flat[-1] == a.max() and (a.ravel()[1:] > a.flat[0]).all()
    a = ref.cell_value(img["max_first_min_last"])
    assert a.flat[0] == a.max() and a.flat[-1] == a.min() and (a.ravel()[:-1] > a.flat[-1]).all()
    assert (img["negative"] < 0).any()
    a = ref.cell_value(img["range_0_255"])
    assert a.min() == 0 and a.max() == 255 and (a != np.floor(a)).any()
    a = ref.cell_value(img["on_and_below_integers"])
    assert a.min() == 0 and a.max() == 510 and (a == np.floor(a)).any() and (a != np.floor(a)).any()
    assert img["one_by_one"].shape == (1, 1) and img["one_by_n"].shape == (13, 1)
    # the entries the reference was seen to hold: not the textbook jet
    seen = {0: (0, 0, 255), 1: (0, 3, 255), 31: (0, 93, 254), 32: (0, 96, 255), 95: (30, 255, 224), 127: (126, 255, 128),
            128: (129, 255, 125), 191: (255, 191, 0), 254: (255, 2, 0), 255: (255, 0, 0)}
    for i, rgb in seen.items():
        assert tuple(golden.lut[i]) == rgb, i


def test_colormap_equals_the_goldens_768_values(host, golden):
    from hpmvs_amd import api
    assert np.array_equal(ref.colormap(), golden.lut)
    assert np.array_equal(host.colormap(), golden.lut)
    lut = api.depth_colormap()   # host only: no device is looked for
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and np.array_equal(lut, golden.lut)


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_equals_cimg_byte_for_byte(golden, name):
    rgb, (m, M) = ref.image(golden.img[name].T, golden.lut)
    assert np.array_equal(rgb, golden.rgb[name])
    v = ref.cell_value(golden.img[name])
    assert m == v.min() and M == v.max()


@pytest.mark.parametrize("name", CASES)
def test_host_compile_of_the_header_equals_cimg_byte_for_byte(host, golden, name):
    rgb, (m, M) = host.image(golden.img[name].T)
    assert np.array_equal(rgb, golden.rgb[name])
    _, (rm, rM) = ref.image(golden.img[name].T, golden.lut)
    assert m == rm and M == rM


def test_an_all_empty_and_a_one_depth_map_are_entry_0_everywhere(golden):
    for n in ("all_empty", "one_depth", "one_by_one"):
        assert (golden.rgb[n] == golden.lut[0]).all(), n


def test_cells_that_are_not_finite_count_as_empty(host, golden):
    a = golden.img["dense_35x23"].T.copy()
    want, rng = ref.image(np.where(np.isin(np.arange(a.size).reshape(a.shape), (5, 77, 300)), ref.MAX_DEPTH, a), golden.lut)
    a.flat[5], a.flat[77], a.flat[300] = np.nan, np.inf, -np.inf
    for rgb, got in (ref.image(a, golden.lut), host.image(a)):
        assert np.array_equal(rgb, want) and got[0] == rng[0] == 0 and got[1] == rng[1]


def test_full_depth_over_odd_sized_levels(host, golden):
    """35 columns over 17 over 8: column 34 returns at level 1 (34 >> 1 = 17), columns 32 .. 33 at level 2 (8 >= 8)"""
    shapes = ref.MAP_SHAPES[0]
    levels = ref.sparse_levels(shapes, 0xF0)
    levels[1][:, :] = np.where(levels[1] == ref.MAX_DEPTH, levels[1], levels[1] - np.float32(10.0))   # (the upper levels win somewhere)
    levels[0][3, 4], levels[0][9, 9], levels[0][20, 2] = np.nan, np.inf, -np.inf
    levels[1][4, 4] = np.nan
    want = ref.combined(levels)
    # by hand, cell by cell
    by_hand = np.full(shapes[0], ref.MAX_DEPTH, np.float32)
    for x in range(shapes[0][0]):
        for y in range(shapes[0][1]):
            d = ref.MAX_DEPTH
            for l, m in enumerate(levels):
                if (x >> l) >= m.shape[0] or (y >> l) >= m.shape[1]:
                    break
                v = m[x >> l, y >> l]
                if np.isfinite(v) and v < d:
                    d = v
            by_hand[x, y] = d
    assert np.array_equal(want, by_hand)
    assert np.array_equal(host.combined(levels), want)
    only0 = ref.cell_depth(levels[0])
    assert np.array_equal(want[34], only0[34]) and not np.array_equal(want[:32], only0[:32])   # the early return was taken
    assert np.array_equal(host.image(want)[0], ref.image(want, golden.lut)[0])


def test_entries_check_arguments_before_the_device():
    from hpmvs_amd import api
    L = api.lib()
    buf = np.zeros(4096, np.uint8)
    n = C.c_size_t(0)
    w, h = C.c_int(), C.c_int()
    assert L.hpmvs_depth_colormap(None) == ref.HPMVS_ERR_ARG
    # no scene: the depth-map entries' own code and message
    assert L.hpmvs_scene_depth_image(None, 0, 0, buf.ctypes.data, buf.nbytes, 0, C.byref(w), C.byref(h), None) == ref.HPMVS_ERR_STATE
    assert "hpmvs_scene_depth_reset" in L.hpmvs_last_error().decode()
    assert L.hpmvs_scene_depth_jpeg(None, 0, ref.COMBINED, 100, buf.ctypes.data, buf.nbytes, C.byref(n)) == ref.HPMVS_ERR_STATE
    assert L.hpmvs_scene_depth_jpeg(None, 0, 0, 100, buf.ctypes.data, buf.nbytes, None) == ref.HPMVS_ERR_ARG
