"""Baseline JPEG decoding on the GPU (kernel_jpeg.hip behind the host's entropy decoder; reference Image::load through
CImg and libjpeg's defaults): Pillow's pixels of tests/golden/g7_jpeg.npz byte for byte, host and device destinations,
agreement with the host restatement on coefficients no encoder produces, refusals, and scenes and a C++ NVM model whose
views are JPEG files against the same scenes built from the decoded pixels."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from jpeg_ref import GUARD, HPMVS_OK, Golden, HostJpeg, mutations

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostJpeg(tmp_path_factory.mktemp("jpeg_host"))


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
def decoded_views(api, golden):
    """the fixture's scene views decoded once by api.jpeg_decode"""
    return [api.jpeg_decode(b) for b in golden.scene_jpg]


def _decode_fenced_host(api, data, w, h):
    raw = np.full(2 * GUARD + 3 * w * h, 0xA5, np.uint8)
    api._chk(api.lib().hpmvs_jpeg_decode(0, data, len(data), raw.ctypes.data + GUARD, 3 * w * h, 0))
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "a guard byte of the host buffer was written"
    return raw[GUARD:-GUARD].reshape(h, w, 3).copy()


def _decode_fenced_device(api, data, w, h):
    import torch
    raw = torch.full((2 * GUARD + 3 * w * h,), 0xA5, dtype=torch.uint8, device="cuda:0")
    api._chk(api.lib().hpmvs_jpeg_decode(0, data, len(data), raw.data_ptr() + GUARD, 3 * w * h, 1))
    raw = raw.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "a guard byte of the device buffer was written"
    return raw[GUARD:-GUARD].reshape(h, w, 3).copy()


def test_decode_equals_pillow_byte_for_byte(api, golden):
    for n in golden.names:
        out = api.jpeg_decode(golden.jpg[n])
        assert out.dtype == np.uint8 and out.shape == golden.rgb[n].shape, n
        assert int((out != golden.rgb[n]).sum()) == 0, f"{n}: {int((out != golden.rgb[n]).sum())} values differ from Pillow {golden.pillow}"


def test_device_destination_equals_host_destination_and_guards_hold(api, golden):
    for n in golden.names:
        w, h = golden.info[n][:2]
        on_host = _decode_fenced_host(api, golden.jpg[n], w, h)
        on_dev = _decode_fenced_device(api, golden.jpg[n], w, h)   # odd widths: the unaligned store path
        assert np.array_equal(on_host, golden.rgb[n]), n
        assert np.array_equal(on_dev, on_host), n
    t = api.jpeg_decode(golden.jpg[golden.names[-1]], on_device=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), golden.rgb[golden.names[-1]])


def test_device_equals_host_restatement_on_mutated_files(api, host, golden):
    """coefficients no encoder produces: the first three mutations of the largest entry that the host decoder accepts"""
    name = "c200x136_420_q85"
    taken = 0
    for m in mutations(golden.jpg[name], seed=golden.names.index(name)):
        rc, info, _ = host.info(m)
        if rc != HPMVS_OK:
            continue
        w, h = info[:2]
        rc, ref, _ = host.decode(m, w, h)
        assert rc == HPMVS_OK
        assert np.array_equal(_decode_fenced_device(api, m, w, h), ref)
        taken += 1
        if taken == 3:
            break
    assert taken == 3


def test_refusals_keep_their_codes_and_leave_the_scene_usable(api, golden, tiny_scene):
    L = api.lib()
    out = np.zeros(3 * 64 * 64, np.uint8)
    v = tiny_scene.views[0]
    h = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(h)))
    try:
        cam = api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, tiny_scene.max_level)
        for n in golden.refuse_names:
            b = golden.refuse_jpg[n]
            assert L.hpmvs_jpeg_decode(0, b, len(b), out.ctypes.data, out.nbytes, 0) == golden.refuse_code[n], n
            assert L.hpmvs_scene_set_view_jpeg(h, 0, b, len(b), C.byref(cam), float(v.f), 0.0) == golden.refuse_code[n], n
            assert golden.refuse_word[n] in L.hpmvs_last_error().decode(), n
        good = golden.scene_jpg[0]
        assert L.hpmvs_scene_set_view_jpeg(h, 1, good, len(good), C.byref(cam), float(v.f), 0.0) == -2   # bad view index
        assert L.hpmvs_scene_set_view_jpeg(h, 0, good, len(good), C.byref(cam), 0.0, 0.1) == -2          # bad f
        api._chk(L.hpmvs_scene_set_view_jpeg(h, 0, good, len(good), C.byref(cam), float(v.f), 0.0))
        api._chk(L.hpmvs_scene_commit(h))
        w, hh = C.c_int(), C.c_int()
        lvl = np.empty((v.height, v.width, 3), np.uint8)
        api._chk(L.hpmvs_scene_get_level(h, 0, 0, lvl.ctypes.data, lvl.nbytes, C.byref(w), C.byref(hh)))
        assert (w.value, hh.value) == (v.width, v.height)
        assert np.array_equal(lvl, api.jpeg_decode(good))
    finally:
        L.hpmvs_scene_destroy(h)


def _levels(sc, n_views):
    out = []
    for i in range(n_views):
        lv, l = [], 0
        while True:
            try:
                lv.append(sc.level(i, l))
            except Exception:
                break
            l += 1
        out.append(lv)
    return out


@pytest.mark.parametrize("k1s", [[0.0, 0.0, 0.0], [0.05, -0.08, 0.0]])
def test_scene_from_jpeg_bytes_equals_scene_from_decoded_arrays(api, golden, tiny_scene, decoded_views, k1s):
    """every level of every view; with k1 != 0 against hpmvs_scene_set_view_distorted on the decoded arrays"""
    assert tiny_scene.n_views == len(golden.scene_jpg)
    as_jpeg = dataclasses.replace(tiny_scene, views=[dataclasses.replace(v, rgb=b if i else bytearray(b), k1=k)
                                                     for i, (v, b, k) in enumerate(zip(tiny_scene.views, golden.scene_jpg, k1s))])
    as_arrays = dataclasses.replace(tiny_scene, views=[dataclasses.replace(v, rgb=a, k1=k)
                                                       for v, a, k in zip(tiny_scene.views, decoded_views, k1s)])
    a = api.Scene(as_jpeg, device=0)
    b = api.Scene(as_arrays, device=0)
    try:
        la, lb = _levels(a, tiny_scene.n_views), _levels(b, tiny_scene.n_views)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert len(x) == len(y) >= 2
            for l, (p, q) in enumerate(zip(x, y)):
                assert np.array_equal(p, q), f"view {i} level {l}"
        assert np.array_equal(la[2][0], decoded_views[2])            # k1 == 0: level 0 is the decode itself
        if k1s[0] != 0.0:
            assert not np.array_equal(la[0][0], decoded_views[0])    # ... and really resampled otherwise
    finally:
        a.close()
        b.close()


def _write_nvm(path, scene, ext, xyz, off, img):
    with open(path, "w") as f:
        f.write("NVM_V3\n\n%d\n" % scene.n_views)
        for i, v in enumerate(scene.views):
            f.write("view%02d.%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g 0 0\n" %
                    (i, ext, v.f, v.q[0], v.q[1], v.q[2], v.q[3], v.c[0], v.c[1], v.c[2]))
        f.write("\n%d\n" % len(xyz))
        for k in range(len(xyz)):
            ms = img[off[k]:off[k + 1]]
            f.write("%.17g %.17g %.17g 128 128 128 %d" % (xyz[k, 0], xyz[k, 1], xyz[k, 2], len(ms)))
            for m in ms:
                f.write(" %d %d 0 0" % (m, k))
            f.write("\n")
        f.write("\n0\n")


def _run_model(exe, d, scene, ext, files, xyz, off, img):
    os.makedirs(d, exist_ok=True)
    for i, data in enumerate(files):
        with open(os.path.join(d, "view%02d.%s" % (i, ext)), "wb") as f:
            f.write(data)
    _write_nvm(os.path.join(d, "scene.nvm"), scene, ext, xyz, off, img)
    subprocess.run([exe, os.path.join(d, "scene.nvm"), os.path.join(d, "out.ply"), os.path.join(d, "copy.nvm"), "2"],
                   check=True, capture_output=True, text=True, timeout=600)
    return open(os.path.join(d, "out.ply"), "rb").read()


def test_cpp_nvm_model_with_jpeg_views(api, golden, tiny_scene, decoded_views, tmp_path):
    """Scene::addCameras on an NVM model that names JPEG files, as VisualSFM writes it: the PLY equals the one of the same
    model whose views are PPM files of the decoded pixels."""
    from hpmvs_amd import synth
    exe = os.path.join(ROOT, "tests", "native", "run_nvm_scene")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), "all"], check=True, capture_output=True)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 300, start_level=2, noise=1.0)
    w, h = golden.scene_size
    ppms = [b"P6\n%d %d\n255\n" % (w, h) + a.tobytes() for a in decoded_views]
    from_jpeg = _run_model(exe, str(tmp_path / "jpg"), tiny_scene, "jpg", golden.scene_jpg, xyz, off, img)
    from_ppm = _run_model(exe, str(tmp_path / "ppm"), tiny_scene, "ppm", ppms, xyz, off, img)
    assert from_jpeg == from_ppm
    n_vertices = int(re.search(rb"element vertex (\d+)", from_jpeg).group(1))
    print(f"\n{n_vertices} vertices reconstructed from the JPEG views")
    assert n_vertices >= 20
