"""The image entry points' early exits, entry by entry: every refusal that is reachable without a device -- a null argument, a
bad size, bad undistortion parameters, overlapping buffers, a bad `entropy` or `subseq_bits` value, a truncated or unsupported
file, a short output, a quality out of range -- with its status code and its text in hpmvs_last_error, in the order the entry
checks them, and HPMVS_ERR_NODEVICE behind them all.  Codes and texts are written out here as the library gave them before
these entries moved to a file of their own (hpmvs_amd/csrc/capi_image.hip); the files are tests/golden/g7_jpeg.npz's."""
import ctypes as C
import threading

import numpy as np
import pytest

from jpeg_ref import Golden

OK, ERR_ARG, ERR_STATE, ERR_NODEVICE, ERR_UNSUPPORTED = 0, -2, -3, -4, -5
AUTO, HOST, DEVICE = 0, 1, 2
NAME, W, H = "c37x29_420_q75", 37, 29
N_COEF = 64 * (6 * 4 + 2 * 3 * 2)      # 4:2:0 at 37 x 29: 3 x 2 MCUs of 16 x 16, luma 6 x 4 blocks, each chroma plane 3 x 2
NO_DEVICE = "no HIP device visible"


@pytest.fixture(scope="module")
def env():
    from hpmvs_amd import api
    g = Golden()
    e = type("Env", (), {})()
    e.api, e.L = api, api.lib()
    e.good = g.jpg[NAME]
    assert g.info[NAME][:2] == (W, H)
    e.cut = g.refuse_jpg["cut_in_entropy_data"]   # the headers parse, the scan ends early: refused by the walk of the scan
    e.eoi = e.good[:-2]                           # likewise, by the scan's end
    e.progressive = g.refuse_jpg["progressive"]   # refused by the header parse
    e.rgb = np.zeros(3 * W * H, np.uint8)
    e.coef = np.zeros(N_COEF, np.int16)
    e.ms = (C.c_float * 16)()
    e.out = np.zeros(4096, np.uint8)
    e.n = C.c_size_t(0)
    e.img = np.zeros(2 * 3 * 16 * 16, np.uint8)   # two 16 x 16 images, one behind the other
    e.xy = np.zeros(2 * 16 * 16, np.float32)
    return e


def _cases(e):
    """[(id, call, code, text)] in the order each entry checks; a text of None: the message is not looked at"""
    L, rgb, cap, good = e.L, e.rgb.ctypes.data, e.rgb.nbytes, e.good
    coef, ms, out, n = e.coef.ctypes.data, e.ms, e.out.ctypes.data, C.byref(e.n)
    a, b = e.img.ctypes.data, e.img.ctypes.data + 3 * 16 * 16
    v = [C.byref(C.c_int()) for _ in range(5)]
    nan, inf = float("nan"), float("inf")
    small = "output buffer smaller than 3 * width * height"
    under8 = "jpeg_encode: a side under 8 pixels is below what the decoder here reads back"
    fk = "f must be finite and > 0, k1 finite"
    cases = [
        ("info null bytes", lambda: L.hpmvs_jpeg_info(None, 10, *v), ERR_ARG, "jpeg_info: null argument"),
        ("info null width", lambda: L.hpmvs_jpeg_info(good, len(good), None, *v[1:]), ERR_ARG, "jpeg_info: null argument"),
        ("info null v_samp", lambda: L.hpmvs_jpeg_info(good, len(good), *v[:4], None), ERR_ARG, "jpeg_info: null argument"),
        ("info truncated", lambda: L.hpmvs_jpeg_info(e.cut, len(e.cut), *v), ERR_ARG, "truncated"),
        ("info no EOI", lambda: L.hpmvs_jpeg_info(e.eoi, len(e.eoi), *v), ERR_ARG, "EOI"),
        ("info one byte", lambda: L.hpmvs_jpeg_info(good, 1, *v), ERR_ARG, "SOI"),
        ("info progressive", lambda: L.hpmvs_jpeg_info(e.progressive, len(e.progressive), *v), ERR_UNSUPPORTED, "progressive"),

        ("decode null bytes", lambda: L.hpmvs_jpeg_decode(0, None, len(good), rgb, cap, 0), ERR_ARG, "jpeg_decode: null argument"),
        ("decode null rgb", lambda: L.hpmvs_jpeg_decode(0, good, len(good), None, cap, 0), ERR_ARG, "jpeg_decode: null argument"),
        ("decode one byte", lambda: L.hpmvs_jpeg_decode(0, good, 1, rgb, cap, 0), ERR_ARG, "SOI"),
        ("decode progressive", lambda: L.hpmvs_jpeg_decode(0, e.progressive, len(e.progressive), rgb, cap, 0), ERR_UNSUPPORTED, "progressive"),
        ("decode short", lambda: L.hpmvs_jpeg_decode(0, good, len(good), rgb, cap - 1, 0), ERR_ARG, "jpeg_decode: " + small),
        # a file whose scan is refused says so before the short buffer, the missing device and the bad device index do
        ("decode truncated and short", lambda: L.hpmvs_jpeg_decode(0, e.cut, len(e.cut), rgb, cap - 1, 0), ERR_ARG, "truncated"),
        ("decode no EOI and short", lambda: L.hpmvs_jpeg_decode(0, e.eoi, len(e.eoi), rgb, 0, 0), ERR_ARG, "EOI"),
        ("decode truncated", lambda: L.hpmvs_jpeg_decode(0, e.cut, len(e.cut), rgb, cap, 0), ERR_ARG, "truncated"),
        ("decode truncated, device 99", lambda: L.hpmvs_jpeg_decode(99, e.cut, len(e.cut), rgb, cap, 0), ERR_ARG, "truncated"),
        ("decode_ex bad entropy 3", lambda: L.hpmvs_jpeg_decode_ex(0, good, len(good), rgb, cap, 0, 3, None), ERR_ARG, "jpeg_decode: bad entropy value"),
        ("decode_ex bad entropy -1", lambda: L.hpmvs_jpeg_decode_ex(0, good, len(good), rgb, cap, 0, -1, None), ERR_ARG, "jpeg_decode: bad entropy value"),
        ("decode_ex null before entropy", lambda: L.hpmvs_jpeg_decode_ex(0, None, len(good), rgb, cap, 0, 3, None), ERR_ARG, "jpeg_decode: null argument"),
        ("decode_ex entropy before file", lambda: L.hpmvs_jpeg_decode_ex(0, e.progressive, len(e.progressive), rgb, cap, 0, 7, None), ERR_ARG,
         "jpeg_decode: bad entropy value"),
        ("decode_ex short", lambda: L.hpmvs_jpeg_decode_ex(0, good, len(good), rgb, cap - 1, 0, DEVICE, None), ERR_ARG, "jpeg_decode: " + small),
        ("decode_ex truncated and short", lambda: L.hpmvs_jpeg_decode_ex(0, e.cut, len(e.cut), rgb, cap - 1, 0, DEVICE, None), ERR_ARG, "truncated"),

        ("coefficients null bytes", lambda: L.hpmvs_jpeg_coefficients(0, None, len(good), HOST, 0, coef, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: null argument"),
        ("coefficients null coef", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), HOST, 0, None, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: null argument"),
        ("coefficients bad entropy", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), 3, 0, coef, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: bad entropy value"),
        ("coefficients subseq_bits 33", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), DEVICE, 33, coef, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: subseq_bits must be 0 or a multiple of 32 from 64 up"),
        ("coefficients subseq_bits 48", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), DEVICE, 48, coef, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: subseq_bits must be 0 or a multiple of 32 from 64 up"),
        ("coefficients subseq_bits 32", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), HOST, 32, coef, N_COEF, None, None), ERR_ARG,
         "jpeg_coefficients: subseq_bits must be 0 or a multiple of 32 from 64 up"),
        ("coefficients one byte", lambda: L.hpmvs_jpeg_coefficients(0, good, 1, HOST, 0, coef, N_COEF, None, None), ERR_ARG, "SOI"),
        ("coefficients progressive", lambda: L.hpmvs_jpeg_coefficients(0, e.progressive, len(e.progressive), HOST, 0, coef, N_COEF, None, None),
         ERR_UNSUPPORTED, "progressive"),
        ("coefficients short", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), HOST, 0, coef, N_COEF - 1, None, None), ERR_ARG,
         "jpeg_coefficients: output buffer smaller than the frame's coefficients"),
        # (this entry walks no scan for an argument error: the short buffer comes before the truncated scan)
        ("coefficients truncated and short", lambda: L.hpmvs_jpeg_coefficients(0, e.cut, len(e.cut), HOST, 0, coef, N_COEF - 1, None, None), ERR_ARG,
         "jpeg_coefficients: output buffer smaller than the frame's coefficients"),

        ("last_decode null", lambda: L.hpmvs_jpeg_last_decode(None, None), ERR_ARG, "jpeg_last_decode: null argument"),

        ("decode_timed null bytes", lambda: L.hpmvs_jpeg_decode_timed(0, None, len(good), rgb, cap, ms), ERR_ARG, "jpeg_decode_timed: null argument"),
        ("decode_timed null rgb", lambda: L.hpmvs_jpeg_decode_timed(0, good, len(good), None, cap, ms), ERR_ARG, "jpeg_decode_timed: null argument"),
        ("decode_timed null ms", lambda: L.hpmvs_jpeg_decode_timed(0, good, len(good), rgb, cap, None), ERR_ARG, "jpeg_decode_timed: null argument"),
        ("decode_timed truncated", lambda: L.hpmvs_jpeg_decode_timed(0, e.cut, len(e.cut), rgb, cap, ms), ERR_ARG, "truncated"),
        ("decode_timed truncated and short", lambda: L.hpmvs_jpeg_decode_timed(0, e.cut, len(e.cut), rgb, cap - 1, ms), ERR_ARG, "truncated"),
        ("decode_timed progressive", lambda: L.hpmvs_jpeg_decode_timed(0, e.progressive, len(e.progressive), rgb, cap, ms), ERR_UNSUPPORTED, "progressive"),
        ("decode_timed short", lambda: L.hpmvs_jpeg_decode_timed(0, good, len(good), rgb, cap - 1, ms), ERR_ARG, "jpeg_decode_timed: " + small),

        ("entropy_timed null bytes", lambda: L.hpmvs_jpeg_entropy_timed(0, None, len(good), rgb, cap, ms), ERR_ARG, "jpeg_entropy_timed: null argument"),
        ("entropy_timed null rgb", lambda: L.hpmvs_jpeg_entropy_timed(0, good, len(good), None, cap, ms), ERR_ARG, "jpeg_entropy_timed: null argument"),
        ("entropy_timed null ms", lambda: L.hpmvs_jpeg_entropy_timed(0, good, len(good), rgb, cap, None), ERR_ARG, "jpeg_entropy_timed: null argument"),
        ("entropy_timed one byte", lambda: L.hpmvs_jpeg_entropy_timed(0, good, 1, rgb, cap, ms), ERR_ARG, "SOI"),
        ("entropy_timed progressive", lambda: L.hpmvs_jpeg_entropy_timed(0, e.progressive, len(e.progressive), rgb, cap, ms), ERR_UNSUPPORTED,
         "progressive"),
        ("entropy_timed short", lambda: L.hpmvs_jpeg_entropy_timed(0, good, len(good), rgb, cap - 1, ms), ERR_ARG, "jpeg_entropy_timed: " + small),
        ("entropy_timed truncated and short", lambda: L.hpmvs_jpeg_entropy_timed(0, e.cut, len(e.cut), rgb, cap - 1, ms), ERR_ARG,
         "jpeg_entropy_timed: " + small),

        ("encode null rgb", lambda: L.hpmvs_jpeg_encode(0, None, 16, 16, 90, out, 4096, n, 0), ERR_ARG, "jpeg_encode: null argument"),
        ("encode null out", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 90, None, 4096, n, 0), ERR_ARG, "jpeg_encode: null argument"),
        ("encode null n", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 90, out, 4096, None, 0), ERR_ARG, "jpeg_encode: null argument"),
        ("encode quality 0", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 0, out, 4096, n, 0), ERR_ARG, "jpeg_encode: quality must be 1 .. 100"),
        ("encode quality 101", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 101, out, 4096, n, 0), ERR_ARG, "jpeg_encode: quality must be 1 .. 100"),
        ("encode width 65536", lambda: L.hpmvs_jpeg_encode(0, a, 65536, 16, 90, out, 4096, n, 0), ERR_ARG, "jpeg_encode: a side above 65535 pixels does not fit a JPEG frame header"),
        ("encode height 0", lambda: L.hpmvs_jpeg_encode(0, a, 16, 0, 90, out, 4096, n, 0), ERR_UNSUPPORTED, under8),
        ("encode width 7", lambda: L.hpmvs_jpeg_encode(0, a, 7, 16, 90, out, 4096, n, 0), ERR_UNSUPPORTED, under8),
        ("encode_timed null ms", lambda: L.hpmvs_jpeg_encode_timed(0, a, 16, 16, 90, out, 4096, n, None), ERR_ARG, "jpeg_encode_timed: null argument"),
        ("encode_timed null rgb", lambda: L.hpmvs_jpeg_encode_timed(0, None, 16, 16, 90, out, 4096, n, ms), ERR_ARG, "jpeg_encode: null argument"),
        ("encode_timed quality 0", lambda: L.hpmvs_jpeg_encode_timed(0, a, 16, 16, 0, out, 4096, n, ms), ERR_ARG, "jpeg_encode: quality must be 1 .. 100"),
        ("encode_timed height 7", lambda: L.hpmvs_jpeg_encode_timed(0, a, 16, 7, 90, out, 4096, n, ms), ERR_UNSUPPORTED, under8),

        ("build_pyramid null src", lambda: L.hpmvs_build_pyramid(0, None, 16, 16, b, 0), ERR_ARG, "build_pyramid: bad argument"),
        ("build_pyramid null dst", lambda: L.hpmvs_build_pyramid(0, a, 16, 16, None, 0), ERR_ARG, "build_pyramid: bad argument"),
        ("build_pyramid width 1", lambda: L.hpmvs_build_pyramid(0, a, 1, 16, b, 0), ERR_ARG, "build_pyramid: bad argument"),
        ("build_pyramid height 1", lambda: L.hpmvs_build_pyramid(0, a, 16, 1, b, 0), ERR_ARG, "build_pyramid: bad argument"),

        ("undistort null src", lambda: L.hpmvs_undistort(0, None, 16, 16, 20.0, 0.1, b, 0), ERR_ARG, "undistort: bad argument"),
        ("undistort null dst", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, 0.1, None, 0), ERR_ARG, "undistort: bad argument"),
        ("undistort width 1", lambda: L.hpmvs_undistort(0, a, 1, 16, 20.0, 0.1, b, 0), ERR_ARG, "undistort: bad argument"),
        ("undistort f 0", lambda: L.hpmvs_undistort(0, a, 16, 16, 0.0, 0.1, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort f negative", lambda: L.hpmvs_undistort(0, a, 16, 16, -5.0, 0.0, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort f nan", lambda: L.hpmvs_undistort(0, a, 16, 16, nan, 0.1, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort f inf", lambda: L.hpmvs_undistort(0, a, 16, 16, inf, 0.1, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort k1 nan", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, nan, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort k1 inf", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, inf, b, 0), ERR_ARG, "undistort: " + fk),
        ("undistort same buffer", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, 0.1, a, 0), ERR_ARG, "undistort: src and dst overlap"),
        ("undistort dst one byte inside src", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, 0.1, b - 1, 0), ERR_ARG, "undistort: src and dst overlap"),
        ("undistort src one byte inside dst", lambda: L.hpmvs_undistort(0, b - 1, 16, 16, 20.0, 0.1, a, 0), ERR_ARG, "undistort: src and dst overlap"),
        ("undistort bad f before overlap", lambda: L.hpmvs_undistort(0, a, 16, 16, 0.0, 0.1, a, 0), ERR_ARG, "undistort: " + fk),

        ("undistort_map null xy", lambda: L.hpmvs_undistort_map(0, 16, 16, 20.0, 0.1, None), ERR_ARG, "undistort_map: bad argument"),
        ("undistort_map height 1", lambda: L.hpmvs_undistort_map(0, 16, 1, 20.0, 0.1, e.xy.ctypes.data), ERR_ARG, "undistort_map: bad argument"),
        ("undistort_map f 0", lambda: L.hpmvs_undistort_map(0, 16, 16, 0.0, 0.1, e.xy.ctypes.data), ERR_ARG, "undistort_map: " + fk),
        ("undistort_map k1 nan", lambda: L.hpmvs_undistort_map(0, 16, 16, 20.0, nan, e.xy.ctypes.data), ERR_ARG, "undistort_map: " + fk),
    ]
    # what every entry that takes a device says behind its last argument check, with arguments nothing is wrong with
    last = [
        ("decode", lambda: L.hpmvs_jpeg_decode(0, good, len(good), rgb, cap, 0)),
        ("decode_ex device", lambda: L.hpmvs_jpeg_decode_ex(0, good, len(good), rgb, cap, 0, DEVICE, None)),
        ("decode_ex host", lambda: L.hpmvs_jpeg_decode_ex(0, good, len(good), rgb, cap, 0, HOST, None)),
        ("decode, device 99", lambda: L.hpmvs_jpeg_decode(99, good, len(good), rgb, cap, 0)),
        ("coefficients", lambda: L.hpmvs_jpeg_coefficients(0, good, len(good), HOST, 0, coef, N_COEF, None, None)),
        ("coefficients truncated", lambda: L.hpmvs_jpeg_coefficients(0, e.cut, len(e.cut), HOST, 64, coef, N_COEF, None, None)),
        ("decode_timed", lambda: L.hpmvs_jpeg_decode_timed(0, good, len(good), rgb, cap, ms)),
        ("entropy_timed", lambda: L.hpmvs_jpeg_entropy_timed(0, good, len(good), rgb, cap, ms)),
        ("entropy_timed truncated", lambda: L.hpmvs_jpeg_entropy_timed(0, e.cut, len(e.cut), rgb, cap, ms)),
        ("encode", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 90, out, 4096, n, 0)),
        ("encode cap 0", lambda: L.hpmvs_jpeg_encode(0, a, 16, 16, 90, out, 0, n, 0)),
        ("encode_timed", lambda: L.hpmvs_jpeg_encode_timed(0, a, 16, 16, 90, out, 4096, n, ms)),
        ("build_pyramid", lambda: L.hpmvs_build_pyramid(0, a, 16, 16, b, 0)),
        ("undistort", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, 0.1, b, 0)),
        ("undistort k1 0", lambda: L.hpmvs_undistort(0, a, 16, 16, 20.0, 0.0, b, 0)),
        ("undistort adjacent buffers", lambda: L.hpmvs_undistort(0, b, 16, 16, 20.0, 0.1, a, 0)),
        ("undistort_map", lambda: L.hpmvs_undistort_map(0, 16, 16, 20.0, 0.1, e.xy.ctypes.data)),
    ]
    return cases, last


def _run(e, call):
    rc = call()
    return rc, e.L.hpmvs_last_error().decode()


def test_every_early_exit_has_its_code_and_its_text(env):
    cases, _ = _cases(env)
    assert len({c[0] for c in cases}) == len(cases)
    wrong = []
    for name, call, code, text in cases:
        rc, msg = _run(env, call)
        if rc != code or (text is not None and text not in msg):
            wrong.append((name, rc, msg))
    assert not wrong, wrong
    # the library's own texts are whole messages, not parts of longer ones
    for name, call, code, text in cases:
        if text and text.split(":")[0] in ("jpeg_info", "jpeg_decode", "jpeg_coefficients", "jpeg_last_decode", "jpeg_decode_timed",
                                           "jpeg_entropy_timed", "jpeg_encode", "jpeg_encode_timed", "build_pyramid", "undistort", "undistort_map"):
            assert _run(env, call)[1] == text, name
    assert not env.rgb.any() and not env.coef.any() and not env.out.any() and not env.img.any() and not env.xy.any()   # nothing was written


def test_no_device_is_reported_last_and_in_the_same_words_everywhere(env):
    _, last = _cases(env)
    assert len(last) == 17
    if env.api.device_count() == 0:   # (with a device these calls succeed: tests/test_gpu_image_entry_points.py)
        for name, call in last:
            assert _run(env, call) == (ERR_NODEVICE, NO_DEVICE), name


def test_encode_bound_is_zero_outside_the_sides_the_encoder_takes(env):
    L = env.L
    for w, h in ((0, 16), (16, 0), (-1, 16), (65536, 16), (16, 65536)):
        assert L.hpmvs_jpeg_encode_bound(w, h) == 0, (w, h)
    # 623 bytes of header; 208 bytes for each of the 6 blocks of a 16 x 16 MCU and one more, every byte stuffed; EOI
    assert L.hpmvs_jpeg_encode_bound(16, 16) == L.hpmvs_jpeg_encode_bound(9, 9) == L.hpmvs_jpeg_encode_bound(1, 1) == 623 + 2 * (6 * 208 + 1) + 2
    assert L.hpmvs_jpeg_encode_bound(17, 9) == 623 + 2 * (12 * 208 + 1) + 2
    assert L.hpmvs_jpeg_encode_bound(65535, 65535) == 623 + 2 * (6 * 4096 * 4096 * 208 + 1) + 2


def test_last_decode_is_per_thread_and_refuses_before_a_threads_first_decode(env):
    got = []

    def fresh_thread():
        used = C.c_int(-7)
        rc = env.L.hpmvs_jpeg_last_decode(C.byref(used), None)
        got.append((rc, env.L.hpmvs_last_error().decode(), used.value))

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == [(ERR_STATE, "jpeg_last_decode: this thread has decoded no JPEG scan yet", -7)]
