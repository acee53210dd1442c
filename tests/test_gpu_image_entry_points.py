"""The image entry points (hpmvs_amd/csrc/capi_image.hip) on the paths no other test walks: the three _timed entries against
their untimed forms (bytes equal, every documented ms slot a time, nothing written behind them), a device index no device
has at every entry that takes one, and a device decode the prescan refuses followed by the decode that falls back to the
host walk -- the path on which the coefficient buffer on the device changes hands."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from jpeg_ref import GUARD, Golden

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, -2, -3
AUTO, HOST, DEVICE = 0, 1, 2
SMALL = "c200x136_420_q85"          # tests/test_gpu_jpeg_entropy.py decodes it on the device
SENTINEL = -12345.678               # what the slots behind the documented ones hold before and after


@pytest.fixture(scope="module")
def golden():
    return Golden()


@pytest.fixture(scope="module")
def api():
    from hpmvs_amd import api as a
    if a.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    return a


def _ms(n_slots):
    return (C.c_float * n_slots)(*([SENTINEL] * n_slots))


def _check_ms(ms, documented):
    sentinel = struct.pack("f", SENTINEL)
    for k, v in enumerate(ms):
        if k < documented:
            assert math.isfinite(v) and v >= 0.0, (k, v)
        else:
            assert struct.pack("f", v) == sentinel, f"ms[{k}] was written"


def _fenced(torch, nbytes):
    return torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


def _inside(dev, nbytes):
    host = dev.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all(), "a guard byte was written"
    return host[GUARD:GUARD + nbytes]


def test_decode_timed_gives_the_untimed_pixels_and_four_times(api, golden):
    import torch
    L = api.lib()
    data, (w, h) = golden.jpg[SMALL], golden.info[SMALL][:2]
    nb = 3 * w * h
    plain, timed = _fenced(torch, nb), _fenced(torch, nb)
    api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), plain.data_ptr() + GUARD, nb, 1, HOST, None))
    ms = _ms(8)
    api._chk(L.hpmvs_jpeg_decode_timed(0, data, len(data), timed.data_ptr() + GUARD, nb, ms))
    assert np.array_equal(_inside(timed, nb), _inside(plain, nb))
    assert np.array_equal(_inside(timed, nb).reshape(h, w, 3), golden.rgb[SMALL])
    _check_ms(ms, 4)


def test_entropy_timed_gives_the_untimed_pixels_twelve_slots_and_the_rounds(api, golden):
    import torch
    L = api.lib()
    data, (w, h) = golden.jpg[SMALL], golden.info[SMALL][:2]
    nb = 3 * w * h
    plain, timed = _fenced(torch, nb), _fenced(torch, nb)
    used = C.c_int(-1)
    api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), plain.data_ptr() + GUARD, nb, 1, DEVICE, C.byref(used)))
    assert used.value == DEVICE
    rounds_plain = C.c_int(-1)
    api._chk(L.hpmvs_jpeg_last_decode(C.byref(used), C.byref(rounds_plain)))
    ms = _ms(16)
    api._chk(L.hpmvs_jpeg_entropy_timed(0, data, len(data), timed.data_ptr() + GUARD, nb, ms))
    assert np.array_equal(_inside(timed, nb), _inside(plain, nb))
    assert np.array_equal(_inside(timed, nb).reshape(h, w, 3), golden.rgb[SMALL])
    _check_ms(ms, 12)
    rounds = C.c_int(-1)
    api._chk(L.hpmvs_jpeg_last_decode(C.byref(used), C.byref(rounds)))
    assert used.value == DEVICE and ms[11] == float(rounds.value) and rounds.value == rounds_plain.value


@pytest.mark.parametrize("w,h", [(16, 16), (17, 9)])
def test_encode_timed_gives_the_untimed_file_and_eight_times(api, w, h):
    import torch
    L = api.lib()
    rgb = np.random.default_rng(w * 100 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(rgb).to("cuda:0")
    cap = L.hpmvs_jpeg_encode_bound(w, h)
    plain, timed = np.full(cap + GUARD, 0xA5, np.uint8), np.full(cap + GUARD, 0xA5, np.uint8)
    n_plain, n_timed = C.c_size_t(0), C.c_size_t(0)
    api._chk(L.hpmvs_jpeg_encode(0, dev.data_ptr(), w, h, 90, plain.ctypes.data, cap, C.byref(n_plain), 1))
    ms = _ms(12)
    api._chk(L.hpmvs_jpeg_encode_timed(0, dev.data_ptr(), w, h, 90, timed.ctypes.data, cap, C.byref(n_timed), ms))
    assert 623 + 2 < n_timed.value == n_plain.value <= cap
    assert np.array_equal(timed, plain) and (timed[n_timed.value:] == 0xA5).all()
    assert bytes(timed[:2]) == b"\xff\xd8" and bytes(timed[n_timed.value - 2:n_timed.value]) == b"\xff\xd9"
    assert api.jpeg_info(bytes(timed[:n_timed.value]))[:2] == (w, h)
    from_host = api.jpeg_encode(rgb, quality=90)          # host pixels, staged through a buffer of the call's own
    assert from_host == bytes(plain[:n_plain.value])
    _check_ms(ms, 8)
    short = np.full(cap, 0xA5, np.uint8)                   # one byte short: the length is reported, nothing is written
    n = C.c_size_t(0)
    assert L.hpmvs_jpeg_encode_timed(0, dev.data_ptr(), w, h, 90, short.ctypes.data, n_plain.value - 1, C.byref(n), _ms(8)) == ERR_ARG
    assert "output buffer too small (%d bytes needed)" % n_plain.value in L.hpmvs_last_error().decode()
    assert n.value == n_plain.value and (short == 0xA5).all()


def test_device_index_99_is_a_bad_argument_at_every_entry_that_takes_a_device(api, golden):
    """no entry hands the index to the runtime: each names itself and refuses, and hpmvs_jpeg_decode of a file whose scan is
    refused still reports the file first"""
    L = api.lib()
    data, (w, h) = golden.jpg[SMALL], golden.info[SMALL][:2]
    rgb = np.zeros(3 * w * h, np.uint8)
    coef = np.zeros(64 * 6 * 13 * 9, np.int16)           # 13 x 9 MCUs of six blocks: at least the frame's coefficients
    img, out = np.zeros(2 * 3 * 16 * 16, np.uint8), np.zeros(4096, np.uint8)
    a, b = img.ctypes.data, img.ctypes.data + 3 * 16 * 16
    xy = np.zeros(2 * 16 * 16, np.float32)
    n, ms, sc = C.c_size_t(0), _ms(16), C.c_void_p()
    one = {k: np.zeros(s, t) for k, s, t in (("kind", 1, np.int32), ("params", 8, np.float64), ("x", 3, np.float64), ("i", 1, np.int32))}
    p = lambda name: one[name].ctypes.data_as(C.c_void_p)
    calls = [
        ("scene_create", lambda: L.hpmvs_scene_create(1, 99, C.byref(sc))),
        ("jpeg_decode", lambda: L.hpmvs_jpeg_decode(99, data, len(data), rgb.ctypes.data, rgb.nbytes, 0)),
        ("jpeg_decode", lambda: L.hpmvs_jpeg_decode_ex(99, data, len(data), rgb.ctypes.data, rgb.nbytes, 0, DEVICE, None)),
        ("jpeg_coefficients", lambda: L.hpmvs_jpeg_coefficients(99, data, len(data), DEVICE, 0, coef.ctypes.data, coef.size, None, None)),
        ("jpeg_decode_timed", lambda: L.hpmvs_jpeg_decode_timed(99, data, len(data), rgb.ctypes.data, rgb.nbytes, ms)),
        ("jpeg_entropy_timed", lambda: L.hpmvs_jpeg_entropy_timed(99, data, len(data), rgb.ctypes.data, rgb.nbytes, ms)),
        ("jpeg_encode", lambda: L.hpmvs_jpeg_encode(99, a, 16, 16, 90, out.ctypes.data, out.nbytes, C.byref(n), 0)),
        ("jpeg_encode", lambda: L.hpmvs_jpeg_encode_timed(99, a, 16, 16, 90, out.ctypes.data, out.nbytes, C.byref(n), ms)),
        ("build_pyramid", lambda: L.hpmvs_build_pyramid(99, a, 16, 16, b, 0)),
        ("build_pyramid", lambda: L.hpmvs_build_pyramid(99, a, 16, 16, b, 1)),
        ("undistort", lambda: L.hpmvs_undistort(99, a, 16, 16, C.c_float(20.0), C.c_float(0.1), b, 0)),
        ("undistort", lambda: L.hpmvs_undistort(99, a, 16, 16, C.c_float(20.0), C.c_float(0.0), b, 0)),
        ("undistort_map", lambda: L.hpmvs_undistort_map(99, 16, 16, C.c_float(20.0), C.c_float(0.1), xy.ctypes.data)),
        ("selftest_bobyqa", lambda: L.hpmvs_selftest_bobyqa(99, 0, None, None, None, None, None, 10, None, None, None, None, None, None, 0)),
        ("selftest_bobyqa", lambda: L.hpmvs_selftest_bobyqa(99, 1, p("kind"), p("params"), p("x"), p("x"), p("x"), 10, p("x"), p("x"), p("i"),
                                                            p("i"), p("i"), None, 0)),
    ]
    for who, call in calls:
        assert call() == ERR_ARG, who
        assert L.hpmvs_last_error().decode() == who + ": bad device index", who
    assert L.hpmvs_build_pyramid(-1, a, 16, 16, b, 0) == ERR_ARG and L.hpmvs_last_error().decode() == "build_pyramid: bad device index"
    assert not rgb.any() and not coef.any() and not img.any() and not out.any() and not xy.any() and not sc.value
    cut = golden.refuse_jpg["cut_in_entropy_data"]       # the headers parse, the scan is refused
    assert L.hpmvs_jpeg_decode(99, cut, len(cut), rgb.ctypes.data, rgb.nbytes, 0) == golden.refuse_code["cut_in_entropy_data"] == ERR_ARG
    assert golden.refuse_word["cut_in_entropy_data"] in L.hpmvs_last_error().decode()
    assert "device index" not in L.hpmvs_last_error().decode()


def _threshold():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hpmvs_amd.h")).read()
    return int(re.search(r"#define HPMVS_JPEG_AUTO_MIN_SCAN_BYTES (\d+)", header).group(1))


def test_a_refused_device_decode_and_the_fallback_behind_it(api, golden):
    """FF FF fill in front of EOI, as tests/test_gpu_jpeg_entropy.py makes the file the prescan refuses; bytes behind EOI,
    which every decoder here ignores, lift it over _AUTO's threshold so that _AUTO tries the device before the host walks"""
    L = api.lib()
    base, (w, h) = golden.jpg[SMALL], golden.info[SMALL][:2]
    assert base[-2:] == b"\xff\xd9"
    data = base[:-2] + b"\xff" + base[-2:] + bytes(_threshold())
    nb = 3 * w * h
    for _ in range(2):   # (twice: nothing of the first pair is left behind for the second)
        raw = np.full(2 * GUARD + nb, 0xA5, np.uint8)
        used = C.c_int(-7)
        assert L.hpmvs_jpeg_decode_ex(0, data, len(data), raw.ctypes.data + GUARD, nb, 0, DEVICE, C.byref(used)) == ERR_STATE
        assert L.hpmvs_last_error().decode().startswith("jpeg: ") and "fill bytes" in L.hpmvs_last_error().decode()
        assert (raw == 0xA5).all() and used.value == -7
        api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), raw.ctypes.data + GUARD, nb, 0, AUTO, C.byref(used)))
        assert used.value == HOST
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
        assert np.array_equal(raw[GUARD:-GUARD].reshape(h, w, 3), golden.rgb[SMALL])
        rounds = C.c_int(-1)
        api._chk(L.hpmvs_jpeg_last_decode(C.byref(used), C.byref(rounds)))
        assert (used.value, rounds.value) == (HOST, 0)
    # and the same file without the fill: _AUTO over the threshold stays on the device, the buffer goes on to the IDCT
    intact = base + bytes(_threshold())
    raw = np.full(2 * GUARD + nb, 0xA5, np.uint8)
    used = C.c_int(-7)
    api._chk(L.hpmvs_jpeg_decode_ex(0, intact, len(intact), raw.ctypes.data + GUARD, nb, 0, AUTO, C.byref(used)))
    assert used.value == DEVICE and np.array_equal(raw[GUARD:-GUARD].reshape(h, w, 3), golden.rgb[SMALL])
