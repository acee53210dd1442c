"""Baseline JPEG encoding, host side: the restatement (hpmvs_amd/csrc/jpeg_enc.hpp compiled by g++: tables, colour conversion,
forward DCT, quantiser, block walk, header writer -- the functions the kernels call) writes Pillow's (libjpeg-turbo's) files of
tests/golden/g8_jpeg_enc.npz byte for byte, the refusals carry their codes, the bound holds, and the C ABI checks its
arguments before it looks for a device."""
import ctypes as C
import os

import numpy as np
import pytest

from jpeg_enc_ref import GOLDEN, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED, HPMVS_OK, Golden, HostJpegEnc

SIZES = [(16, 16), (8, 8), (24, 40), (17, 9), (40, 24), (33, 10), (250, 130), (9, 33)]   # (W, H)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostJpegEnc(tmp_path_factory.mktemp("jpeg_enc_host"))


@pytest.fixture(scope="module")
def golden():
    return Golden()


def test_fixture_is_what_the_issue_lists(golden):
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    assert golden.pillow and golden.libjpeg
    for w, h in SIZES:
        for kind in ("noise", "smooth"):
            for q in (100, 90, 50, 10):
                n = "%s_%dx%d_q%d" % (kind, w, h, q)
                assert golden.rgb[n].shape == (h, w, 3) and golden.quality[n] == q
    assert {"checker_56x40_q100", "constant_35x21_q100"} <= set(golden.names)
    assert len(golden.names) == 67 and len(golden.decoded) == 2
    chk = golden.rgb["checker_56x40_q100"]
    assert set(np.unique(chk)) == {0, 255} and (chk[:8, :8] == chk[0, 0]).all() and chk[0, 8, 0] != chk[0, 0, 0]


def test_host_restatement_writes_pillows_files_byte_for_byte(host, golden):
    for n in golden.names:
        rc, data, _, msg, intact = host.encode(golden.rgb[n], golden.quality[n])
        assert rc == HPMVS_OK and intact, (n, msg)
        assert data == golden.jpg[n], f"{n}: differs from the file of Pillow {golden.pillow} / libjpeg {golden.libjpeg}"


def test_fixture_covers_the_encoders_paths(host, golden):
    """what tests/golden/make_golden_jpeg_enc.py asserted when it wrote the file, counted again from the files"""
    seen = dict.fromkeys(("stuffed", "zrl", "dc10", "pad", "right", "bottom"), 0)
    for n in golden.names:
        _, data, st, _, _ = host.encode(golden.rgb[n], golden.quality[n])
        seen["stuffed"] += st["stuffed"] > 0 and b"\xff\x00" in data[623:]
        seen["zrl"] += st["zrl"] > 0
        seen["dc10"] += st["dc_category"] >= 10
        seen["pad"] += st["pad_bits"] > 0
        seen["right"] += st["right_dummies"] > 0
        seen["bottom"] += st["bottom_dummies"] > 0
    assert all(v > 0 for v in seen.values()), seen
    heights = {golden.rgb[n].shape[0] for n in golden.names}
    assert any(h % 2 == 0 and h % 16 for h in heights) and any(h % 2 for h in heights)
    _, _, st, _, _ = host.encode(golden.rgb["noise_8x8_q100"], 100)
    assert st["right_dummies"] == 1 and st["bottom_dummies"] == 1   # (and the fourth block is both)


def test_refusals_return_their_codes(host):
    px = np.zeros((16, 16, 3), np.uint8)
    for q in (0, -1, 101):
        rc, _, _, msg, intact = host.encode(px, q)
        assert rc == HPMVS_ERR_ARG and "quality" in msg and intact
    for shape in ((16, 7, 3), (7, 16, 3), (1, 1, 3)):
        rc, _, _, msg, intact = host.encode(np.zeros(shape, np.uint8), 90)
        assert rc == HPMVS_ERR_UNSUPPORTED and "8 pixels" in msg and intact
    rc, _, _, msg, _ = host.encode(np.zeros((8, 65536, 3), np.uint8), 90)
    assert rc == HPMVS_ERR_ARG and "65535" in msg
    rc, data, _, _, _ = host.encode(np.zeros((8, 8, 3), np.uint8), 1)
    assert rc == HPMVS_OK and data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"


def test_short_buffer_is_refused_before_any_write(host, golden):
    n = "noise_17x9_q90"
    size = len(golden.jpg[n])
    rc, _, _, msg, untouched = host.encode(golden.rgb[n], 90, cap=size - 1)
    assert rc == HPMVS_ERR_ARG and "too small" in msg and untouched
    rc, data, _, _, intact = host.encode(golden.rgb[n], 90, cap=size)   # exactly n bytes between the fences
    assert rc == HPMVS_OK and intact and data == golden.jpg[n]


def test_bound_covers_every_file(host, golden):
    from hpmvs_amd import api
    for n in golden.names:
        h, w = golden.rgb[n].shape[:2]
        assert host.bound(w, h) >= len(golden.jpg[n]), n
        assert api.jpeg_encode_bound(w, h) == host.bound(w, h)
    # the largest file an 8x8 image can have: noise chosen block by block is below the bound, and the bound is not absurd
    assert 623 + 2 < host.bound(8, 8) <= 623 + 2 + 2 * (6 * 208 + 1)
    assert api.jpeg_encode_bound(0, 8) == 0 and api.jpeg_encode_bound(8, 65536) == 0
    assert api.jpeg_encode_bound(65535, 65535) == 623 + 2 + 2 * (6 * 4096 * 4096 * 208 + 1)   # (needs 64 bits)


def test_entries_check_arguments_before_the_device(golden):
    from hpmvs_amd import api
    L = api.lib()
    px = np.ascontiguousarray(golden.rgb["noise_16x16_q90"])
    out = np.zeros(api.jpeg_encode_bound(16, 16), np.uint8)
    n = C.c_size_t(0)
    enc = lambda rgb, w, h, q, o, cap, nn: L.hpmvs_jpeg_encode(0, rgb, w, h, q, o, cap, nn, 0)
    assert enc(None, 16, 16, 90, out.ctypes.data, out.nbytes, C.byref(n)) == HPMVS_ERR_ARG
    assert enc(px.ctypes.data, 16, 16, 90, None, out.nbytes, C.byref(n)) == HPMVS_ERR_ARG
    assert enc(px.ctypes.data, 16, 16, 90, out.ctypes.data, out.nbytes, None) == HPMVS_ERR_ARG
    for q in (0, 101):
        assert enc(px.ctypes.data, 16, 16, q, out.ctypes.data, out.nbytes, C.byref(n)) == HPMVS_ERR_ARG
        assert "quality" in L.hpmvs_last_error().decode()
    assert enc(px.ctypes.data, 65536, 8, 90, out.ctypes.data, out.nbytes, C.byref(n)) == HPMVS_ERR_ARG
    assert enc(px.ctypes.data, 7, 16, 90, out.ctypes.data, out.nbytes, C.byref(n)) == HPMVS_ERR_UNSUPPORTED
    assert "8 pixels" in L.hpmvs_last_error().decode()
    assert L.hpmvs_scene_get_level_jpeg(None, 0, 0, 100, out.ctypes.data, out.nbytes, C.byref(n)) == HPMVS_ERR_ARG
    if api.device_count() == 0:
        assert enc(px.ctypes.data, 16, 16, 90, out.ctypes.data, out.nbytes, C.byref(n)) == -4   # HPMVS_ERR_NODEVICE
        with pytest.raises(api.HpmvsError):
            api.jpeg_encode(px)
