"""Baseline JPEG encoding on the GPU (kernel_jpeg_encode.hip; reference Scene::saveAsNVM through CImg's save_jpeg and
libjpeg's defaults): Pillow's files of tests/golden/g8_jpeg_enc.npz byte for byte, host and device inputs, a tight output
buffer between fences, a scene's levels encoded where they lie, the decoder reading the files back, and two threads at once."""
import ctypes as C
import dataclasses
import threading

import numpy as np
import pytest

from jpeg_enc_ref import GUARD, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED, Golden
from jpeg_ref import Golden as DecodeGolden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return Golden()


@pytest.fixture(scope="module")
def api():
    from hpmvs_amd import api as a
    if a.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    return a


@pytest.fixture(scope="module")
def encoded(api, golden):
    """every golden input encoded once by api.jpeg_encode"""
    return {n: api.jpeg_encode(golden.rgb[n], golden.quality[n]) for n in golden.names}


def test_encode_equals_pillow_byte_for_byte(golden, encoded):
    for n in golden.names:
        got, want = encoded[n], golden.jpg[n]
        assert isinstance(got, bytes)
        if got != want:
            first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            pytest.fail(f"{n}: {len(got)} bytes for Pillow {golden.pillow}'s {len(want)}, first difference at byte {first}")


def test_device_input_equals_host_input(api, golden, encoded):
    import torch
    for n in golden.names:
        t = torch.from_numpy(np.ascontiguousarray(golden.rgb[n])).to("cuda:0")
        assert api.jpeg_encode(t, golden.quality[n]) == encoded[n], n
    # a view into a larger device buffer at an odd byte offset: the unaligned pixel loads
    a = golden.rgb["noise_24x40_q90"]
    raw = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda:0")
    raw[1:1 + a.size] = torch.from_numpy(a.reshape(-1)).to("cuda:0")
    out = np.empty(api.jpeg_encode_bound(24, 40), np.uint8)
    n = C.c_size_t(0)
    api._chk(api.lib().hpmvs_jpeg_encode(0, raw.data_ptr() + 1, 24, 40, 90, out.ctypes.data, out.nbytes, C.byref(n), 1))
    assert out[:n.value].tobytes() == encoded["noise_24x40_q90"]


def test_tight_buffer_between_fences_and_one_byte_short(api, golden, encoded):
    L = api.lib()
    for name in ("noise_17x9_q90", "smooth_250x130_q100", "noise_8x8_q10"):
        px = np.ascontiguousarray(golden.rgb[name])
        h, w = px.shape[:2]
        size = len(encoded[name])
        raw = np.full(2 * GUARD + size, 0xA5, np.uint8)
        n = C.c_size_t(0)
        api._chk(L.hpmvs_jpeg_encode(0, px.ctypes.data, w, h, golden.quality[name], raw.ctypes.data + GUARD, size, C.byref(n), 0))
        assert n.value == size and raw[GUARD:GUARD + size].tobytes() == encoded[name]
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + size:] == 0xA5).all(), "a guard byte was written"
        raw[:] = 0xA5
        n = C.c_size_t(0)
        rc = L.hpmvs_jpeg_encode(0, px.ctypes.data, w, h, golden.quality[name], raw.ctypes.data + GUARD, size - 1, C.byref(n), 0)
        assert rc == HPMVS_ERR_ARG and "too small" in L.hpmvs_last_error().decode()
        assert n.value == size                        # the length a second call needs
        assert (raw[GUARD + size - 1:] == 0xA5).all(), "bytes behind cap were written"
        assert (raw == 0xA5).all()                    # (in fact nothing is written at all)


def test_refusals_on_the_device_path(api):
    px = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(api.HpmvsError, match="error %d: .*quality" % HPMVS_ERR_ARG):
        api.jpeg_encode(px, quality=0)
    with pytest.raises(api.HpmvsError, match="error %d: .*8 pixels" % HPMVS_ERR_UNSUPPORTED):
        api.jpeg_encode(np.zeros((7, 16, 3), np.uint8))
    with pytest.raises(api.HpmvsError, match="uint8"):
        api.jpeg_encode(np.zeros((16, 16), np.uint8))


@pytest.mark.parametrize("k1s", [[0.0, 0.0, 0.0], [0.05, -0.08, 0.0]])
def test_scene_levels_are_encoded_where_they_lie(api, tiny_scene, k1s):
    """the golden scene of g7_jpeg.npz (views given as JPEG bytes), levels 0 and 2; with k1 != 0 level 0 holds the undistorted
    pixels, and those are what the file holds"""
    g7 = DecodeGolden()
    sc_in = dataclasses.replace(tiny_scene, views=[dataclasses.replace(v, rgb=b, k1=k)
                                                   for v, b, k in zip(tiny_scene.views, g7.scene_jpg, k1s)])
    sc = api.Scene(sc_in, device=0)
    try:
        for v in range(tiny_scene.n_views):
            for level in (0, 2):
                px = sc.level(v, level)
                assert sc.level_jpeg(v, level) == api.jpeg_encode(px), (v, level)
            assert sc.level_jpeg(v, 2, quality=90) == api.jpeg_encode(sc.level(v, 2), quality=90)
        if k1s[0] != 0.0:
            raw = api.jpeg_decode(g7.scene_jpg[0])
            assert not np.array_equal(sc.level(0, 0), raw)             # the level really is resampled
            assert sc.level_jpeg(0, 0) != api.jpeg_encode(raw)
        # sizes are reported the way hpmvs_scene_get_level reports them; a bad level or quality is refused
        n = C.c_size_t(0)
        api._chk(api.lib().hpmvs_scene_get_level_jpeg(sc.h, 0, 0, 100, None, 0, C.byref(n)))
        w, h = g7.scene_size
        assert n.value == api.jpeg_encode_bound(w, h)
        assert api.lib().hpmvs_scene_get_level_jpeg(sc.h, 0, 99, 100, None, 0, C.byref(n)) == HPMVS_ERR_ARG
        assert api.lib().hpmvs_scene_get_level_jpeg(sc.h, 0, 0, 101, None, 0, C.byref(n)) == HPMVS_ERR_ARG
        assert api.lib().hpmvs_scene_get_level_jpeg(sc.h, 3, 0, 100, None, 0, C.byref(n)) == HPMVS_ERR_ARG
    finally:
        sc.close()


def test_decoder_reads_the_files_back_as_pillow_does(api, golden, encoded):
    assert len(golden.decoded) == 2
    for n, want in golden.decoded.items():
        got = api.jpeg_decode(encoded[n])
        assert got.shape == want.shape and int((got != want).sum()) == 0, n


def test_two_threads_at_once_give_the_same_bytes(api, golden, encoded):
    names = ["smooth_250x130_q100", "noise_250x130_q90"]
    out = {}

    def work(k):
        try:
            out[k] = [api.jpeg_encode(golden.rgb[n], golden.quality[n]) for _ in range(4) for n in names]
        except Exception as e:   # reported by the assert below
            out[k] = e

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    want = [encoded[n] for _ in range(4) for n in names]
    assert out[0] == want and out[1] == want
