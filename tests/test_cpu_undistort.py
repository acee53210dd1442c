"""Level-0 radial undistortion, host side: the restatement (hpmvs_amd/csrc/undistort.hpp compiled by g++) equals the
reference's own Image::undistort (tests/golden/g6_undistort.npz, made by tests/golden/make_golden_undistort.py from
src/hpmvs/Image.cpp:68-146) on every pixel it writes, and writes exactly the pixels it writes.  The C ABI's argument
checks run before any device is touched."""
import os

import numpy as np
import pytest

from undistort_ref import GOLDEN, HostUndistort, golden_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPMVS_ERR_ARG, HPMVS_ERR_NODEVICE = -2, -4


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostUndistort(tmp_path_factory.mktemp("undistort_host"))


def test_golden_fixture_covers_both_signs_and_regimes():
    assert os.path.getsize(GOLDEN) < 2 * 1024 * 1024
    cases = golden_cases()
    k1s = sorted({k1 for _, _, k1, _, _ in cases})
    assert min(k1s) <= -1.0 and max(k1s) >= 0.3 and any(0 < k < 0.01 for k in k1s)
    sizes = {img.shape[:2] for img, _, _, _, _ in cases}
    assert any(h % 2 and w % 2 for h, w in sizes) and any(h % 2 == 0 and w % 2 == 0 for h, w in sizes)
    # some pixels are left unwritten by the reference for every k1 < 0
    assert all((~wr).any() for _, _, k1, _, wr in cases if k1 < 0)


def test_host_restatement_equals_reference_undistort(host):
    for n, (img, f, k1, ref, written) in enumerate(golden_cases()):
        out, wr = host.image(img, f, k1)
        assert np.array_equal(wr, written), f"case {n}: written mask differs at {int((wr != written).sum())} pixels"
        assert np.array_equal(out[written], ref[written]), f"case {n} (f={f}, k1={k1}): pixel values differ"
        assert not out[~written].any()


def test_host_restatement_threads_agree(host):
    img, f, k1, _, _ = golden_cases()[17]
    a, wa = host.image(img, f, k1, threads=1)
    b, wb = host.image(img, f, k1, threads=7)
    assert np.array_equal(a, b) and np.array_equal(wa, wb)


def test_k1_negative_large_reaches_the_real_root_regime(host):
    """k1 = -1: the corners have t12 >= 0 (real square root), the centre t12 < 0; both sampled points are finite."""
    k1, f = -1.0, 288.0
    r2 = lambda x, y: ((x - 160) / f) ** 2 + ((y - 120) / f) ** 2
    assert abs(k1) * r2(0, 0) >= 4 / 27 > abs(k1) * r2(150, 110)   # t12 >= 0 at the corner, < 0 near the centre
    xy = host.map(320, 240, f, k1)
    assert np.isfinite(xy[110, 150]).all() and np.isfinite(xy[0, 0]).all()


def test_undistort_entries_reject_bad_parameters():
    from hpmvs_amd import api
    L = api.lib()
    img = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros_like(img)
    xy = np.zeros((8, 8, 2), np.float32)
    for f, k1 in [(0.0, 0.1), (-5.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (10.0, float("nan")),
                  (10.0, float("inf")), (10.0, float("-inf"))]:
        assert L.hpmvs_undistort(0, img.ctypes.data, 8, 8, f, k1, out.ctypes.data, 0) == HPMVS_ERR_ARG
        assert L.hpmvs_undistort_map(0, 8, 8, f, k1, xy.ctypes.data) == HPMVS_ERR_ARG
        assert L.hpmvs_scene_set_view_distorted(None, 0, 8, 8, img.ctypes.data, 0, None, f, k1) == HPMVS_ERR_ARG
    assert L.hpmvs_undistort(0, None, 8, 8, 10.0, 0.1, out.ctypes.data, 0) == HPMVS_ERR_ARG
    assert L.hpmvs_undistort(0, img.ctypes.data, 8, 8, 10.0, 0.1, img.ctypes.data, 0) == HPMVS_ERR_ARG  # in place
    assert L.hpmvs_undistort_map(0, 8, 8, 10.0, 0.1, None) == HPMVS_ERR_ARG
    if api.device_count() == 0:
        assert L.hpmvs_undistort(0, img.ctypes.data, 8, 8, 10.0, 0.1, out.ctypes.data, 0) == HPMVS_ERR_NODEVICE
        assert L.hpmvs_undistort_map(0, 8, 8, 10.0, 0.1, xy.ctypes.data) == HPMVS_ERR_NODEVICE
