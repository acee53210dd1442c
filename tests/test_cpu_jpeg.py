"""Baseline JPEG decoding, host side: the restatement (hpmvs_amd/csrc/jpeg.hpp compiled by g++: parser, entropy decoder
and the arithmetic the kernels call) equals Pillow's (libjpeg-turbo's) pixels of tests/golden/g7_jpeg.npz byte for byte,
the library's host entries answer and refuse as documented, hostile files end in an error or a result and never in an
out-of-bounds access, and the C ABI checks arguments and the file before it looks for a device."""
import ctypes as C
import os

import numpy as np
import pytest

from jpeg_ref import (GOLDEN, GUARD, HPMVS_ERR_ARG, HPMVS_ERR_NODEVICE, HPMVS_ERR_UNSUPPORTED, HPMVS_OK, Golden, HostJpeg,
                      mutations)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostJpeg(tmp_path_factory.mktemp("jpeg_host"))


@pytest.fixture(scope="module")
def golden():
    return Golden()


def test_fixture_is_what_the_issue_lists(golden):
    assert os.path.getsize(GOLDEN) < 700 * 1024
    assert golden.pillow and golden.libjpeg
    assert len(golden.names) == 13 and len(golden.refuse_names) == 5 and len(golden.scene_jpg) == 3
    samplings = {golden.info[n][2:] for n in golden.names}
    assert samplings == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    assert any(golden.info[n][0] % 16 and golden.info[n][1] % 16 for n in golden.names)
    q1 = golden.rgb["c64x48_420_q1"]
    assert q1.min() == 0 and q1.max() == 255   # both clamps are reached


def test_host_restatement_equals_pillow_byte_for_byte(host, golden):
    for n in golden.names:
        w, h = golden.info[n][:2]
        rc, rgb, intact = host.decode(golden.jpg[n], w, h)
        assert rc == HPMVS_OK and intact, n
        assert rgb.shape == golden.rgb[n].shape
        assert int((rgb != golden.rgb[n]).sum()) == 0, f"{n}: {int((rgb != golden.rgb[n]).sum())} values differ from Pillow {golden.pillow}"


def test_grayscale_is_written_as_equal_channels(host, golden):
    w, h = golden.info["g19x21_q85"][:2]
    _, rgb, _ = host.decode(golden.jpg["g19x21_q85"], w, h)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 0], rgb[..., 2])


def test_jpeg_info_answers_every_entry(host, golden):
    from hpmvs_amd import api
    for n in golden.names:
        assert api.jpeg_info(golden.jpg[n]) == golden.info[n], n
        assert host.info(golden.jpg[n])[1] == golden.info[n], n
    w, h = golden.scene_size
    for b in golden.scene_jpg:
        assert api.jpeg_info(b) == (w, h, 3, 2, 2)
        assert api.jpeg_info(bytearray(b)) == (w, h, 3, 2, 2)


def test_refusals_carry_their_code_and_reason(host, golden):
    from hpmvs_amd import api
    L = api.lib()
    out = np.zeros(3 * 64 * 64, np.uint8)
    v = [C.c_int() for _ in range(5)]
    for n in golden.refuse_names:
        b = golden.refuse_jpg[n]
        assert L.hpmvs_jpeg_info(b, len(b), *[C.byref(x) for x in v]) == golden.refuse_code[n], n
        assert golden.refuse_word[n] in L.hpmvs_last_error().decode(), (n, L.hpmvs_last_error())
        # the decoder refuses the file before it looks for a device
        assert L.hpmvs_jpeg_decode(0, b, len(b), out.ctypes.data, out.nbytes, 0) == golden.refuse_code[n], n
        assert golden.refuse_word[n] in L.hpmvs_last_error().decode(), (n, L.hpmvs_last_error())
        rc, _, msg = host.info(b)
        assert rc == golden.refuse_code[n] and golden.refuse_word[n] in msg, (n, msg)
        with pytest.raises(api.HpmvsError):
            api.jpeg_info(b)
    assert {golden.refuse_code[n] for n in golden.refuse_names} == {HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED}


def _patched(data, marker, offset, value):
    b = bytearray(data)
    b[data.index(marker) + offset] = value
    return bytes(b)


def test_further_refusals_by_header_surgery(host, golden):
    base = golden.jpg["c37x29_420_q75"]
    cases = [
        (_patched(base, b"\xff\xc0", 4, 12), HPMVS_ERR_UNSUPPORTED, "12-bit"),
        (_patched(base, b"\xff\xc0", 11, 0x41), HPMVS_ERR_UNSUPPORTED, "sampling"),        # luma 4x1
        (_patched(base, b"\xff\xc0", 14, 0x21), HPMVS_ERR_UNSUPPORTED, "sampling"),        # chroma 2x1
        (_patched(base, b"\xff\xdb", 4, 0x10), HPMVS_ERR_UNSUPPORTED, "16-bit"),
        (_patched(base, b"\xff\xc0", 1, 0xC9), HPMVS_ERR_UNSUPPORTED, "arithmetic"),
        (_patched(base, b"\xff\xc0", 1, 0xC3), HPMVS_ERR_UNSUPPORTED, "lossless"),
        (_patched(_patched(base, b"\xff\xc0", 7, 0), b"\xff\xc0", 8, 7), HPMVS_ERR_UNSUPPORTED, "smaller than 8"),
        (base[:-2], HPMVS_ERR_ARG, "EOI"),
        (b"P6\n8 8\n255\n" + bytes(192), HPMVS_ERR_ARG, "SOI"),
    ]
    # component ids 'R', 'G', 'B' and no JFIF segment: what libjpeg decodes without a colour transform
    sof = base.index(b"\xff\xc0")
    rgb_ids = bytearray(base)
    rgb_ids[base.index(b"JFIF")] = ord("X")
    sos = base.index(b"\xff\xda")
    for k, c in enumerate(b"RGB"):
        rgb_ids[sof + 10 + 3 * k] = c
        rgb_ids[sos + 5 + 2 * k] = c
    cases.append((bytes(rgb_ids), HPMVS_ERR_UNSUPPORTED, "RGB"))
    for b, code, word in cases:
        rc, _, msg = host.info(b)
        assert rc == code and word in msg, (code, word, rc, msg)


def test_mutated_files_end_in_a_result_or_an_error(host, golden):
    """200 single-byte overwrites and 20 truncations of every supported entry: the process survives, the status is OK or
    an error, and an accepted file leaves the fences around its output alone."""
    n_ok = n_err = 0
    for k, name in enumerate(golden.names):
        for m in mutations(golden.jpg[name], seed=k):
            rc, info, _ = host.info(m)
            assert rc in (HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED)
            if rc != HPMVS_OK:
                n_err += 1
                w, h = golden.info[name][:2]
            else:
                w, h = info[:2]
                if w * h > 1 << 22:   # a width byte was hit: the file cannot hold that many blocks, so this never happens
                    pytest.fail(f"{name}: a mutated header of {w} x {h} was accepted")
            rc2, rgb, intact = host.decode(m, w, h)
            assert rc2 == rc, "info and decode disagree on a file"
            assert intact
            n_ok += rc2 == HPMVS_OK
    print(f"\n{n_ok} mutated files accepted, {n_err} refused")
    assert n_ok > 100 and n_err > 100   # both outcomes were exercised


def test_short_buffer_is_refused_before_any_write(host, golden):
    name = golden.names[1]
    w, h = golden.info[name][:2]
    raw = np.full(3 * w * h + 2 * GUARD, 0xA5, np.uint8)
    rc, msg = host.decode_into(golden.jpg[name], raw.ctypes.data + GUARD, 3 * w * h - 1)
    assert rc == HPMVS_ERR_ARG and (raw == 0xA5).all()


def test_entries_check_arguments_and_the_file_before_the_device(golden):
    from hpmvs_amd import api
    L = api.lib()
    name = golden.names[1]
    b = golden.jpg[name]
    w, h = golden.info[name][:2]
    out = np.zeros(3 * w * h, np.uint8)
    assert L.hpmvs_jpeg_decode(0, None, len(b), out.ctypes.data, out.nbytes, 0) == HPMVS_ERR_ARG
    assert L.hpmvs_jpeg_decode(0, b, len(b), None, out.nbytes, 0) == HPMVS_ERR_ARG
    assert L.hpmvs_jpeg_decode(0, b, len(b), out.ctypes.data, out.nbytes - 1, 0) == HPMVS_ERR_ARG
    assert "smaller" in L.hpmvs_last_error().decode()
    assert L.hpmvs_jpeg_decode(0, b, 1, out.ctypes.data, out.nbytes, 0) == HPMVS_ERR_ARG
    v = [C.c_int() for _ in range(5)]
    assert L.hpmvs_jpeg_info(None, 10, *[C.byref(x) for x in v]) == HPMVS_ERR_ARG
    assert L.hpmvs_jpeg_info(b, len(b), None, *[C.byref(x) for x in v[1:]]) == HPMVS_ERR_ARG
    cam = api.camera_from_nvm(500.0, [1, 0, 0, 0], [0, 0, 0], w, h, 1)
    assert L.hpmvs_scene_set_view_jpeg(None, 0, b, len(b), C.byref(cam), 500.0, 0.0) == HPMVS_ERR_ARG
    for f, k1 in [(0.0, 0.1), (-5.0, 0.0), (float("nan"), 0.1), (float("inf"), 0.0), (10.0, float("nan")), (10.0, float("inf"))]:
        assert L.hpmvs_scene_set_view_jpeg(None, 0, b, len(b), C.byref(cam), f, k1) == HPMVS_ERR_ARG
    if api.device_count() == 0:
        assert L.hpmvs_jpeg_decode(0, b, len(b), out.ctypes.data, out.nbytes, 0) == HPMVS_ERR_NODEVICE
        with pytest.raises(api.HpmvsError):
            api.jpeg_decode(b)
