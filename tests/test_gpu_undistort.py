"""Level-0 radial undistortion on the GPU (kernel_undistort.hip; reference Image::undistort, src/hpmvs/Image.cpp:68-146):
the reference's own output (tests/golden/g6_undistort.npz), full-size maps against the host restatement, scene and
C++-path equivalence with host-undistorted views, and the sign convention of k1 checked without the restatement."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from undistort_ref import HostUndistort, golden_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPMVS_ERR_ARG = -2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostUndistort(tmp_path_factory.mktemp("undistort_host"))


@pytest.fixture(scope="module")
def api():
    from hpmvs_amd import api as a
    if a.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    return a


def test_undistort_equals_reference_golden(api):
    for n, (img, f, k1, ref, written) in enumerate(golden_cases()):
        out = api.undistort(img, f, k1)
        assert np.array_equal(out[written], ref[written]), f"case {n} (f={f}, k1={k1}): {int((out != ref)[written].any(-1).sum())} pixels differ"
        assert not out[~written].any(), f"case {n}: an unwritten pixel is not 0"


def test_undistort_device_pointers_equal_host_pointers(api):
    import torch
    img, f, k1, ref, written = golden_cases()[16]
    out = api.undistort(torch.from_numpy(img).to("cuda:0"), f, k1).cpu().numpy()
    assert np.array_equal(out, api.undistort(img, f, k1))


def _scene_levels_via_distorted(api, scene, k1s):
    """hpmvs_scene_set_view_distorted for every view (k1s[i] per view), levels read back"""
    L = api.lib()
    h = C.c_void_p()
    api._chk(L.hpmvs_scene_create(scene.n_views, 0, C.byref(h)))
    try:
        for i, v in enumerate(scene.views):
            cam = api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, scene.max_level)
            rgb = np.ascontiguousarray(v.rgb, dtype=np.uint8)
            api._chk(L.hpmvs_scene_set_view_distorted(h, i, v.width, v.height, rgb.ctypes.data, 0, C.byref(cam),
                                                      float(v.f), float(k1s[i])))
        out = []
        for i in range(scene.n_views):
            lv, l = [], 0
            while True:
                w, hh = C.c_int(), C.c_int()
                if L.hpmvs_scene_get_level(h, i, l, None, 0, C.byref(w), C.byref(hh)) != 0:
                    break
                a = np.empty((hh.value, w.value, 3), np.uint8)
                api._chk(L.hpmvs_scene_get_level(h, i, l, a.ctypes.data, a.nbytes, C.byref(w), C.byref(hh)))
                lv.append(a)
                l += 1
            out.append(lv)
        return out
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


def test_k1_zero_is_the_identity(api, tiny_scene):
    img = np.ascontiguousarray(tiny_scene.views[0].rgb)
    assert np.array_equal(api.undistort(img, tiny_scene.views[0].f, 0.0), img)
    via_distorted = _scene_levels_via_distorted(api, tiny_scene, [0.0] * tiny_scene.n_views)
    sc = api.Scene(tiny_scene, device=0)
    try:
        plain = _levels(sc, tiny_scene.n_views)
    finally:
        sc.close()
    assert len(plain[0]) >= 2
    for a, b in zip(plain, via_distorted):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


FULL = [(3840, 2160, 1.0, 0.05), (3840, 2160, 1.0, -0.05), (3840, 2160, 0.9, -1.0), (3840, 2160, 1.1, 1e-3),
        (1919, 1081, 1.2, 0.3), (1919, 1081, 0.9, -0.3), (1919, 1081, 1.0, -1.0)]


@pytest.mark.parametrize("w,h,ff,k1", FULL)
def test_full_size_map_against_host_restatement(api, host, w, h, ff, k1):
    f = float(np.float32(ff * w))
    dev = api.undistort_map(w, h, f, k1)
    ref = host.map(w, h, f, k1)
    both_nan = np.isnan(dev) & np.isnan(ref)
    same = (dev.view(np.uint32) == ref.view(np.uint32)) | both_nan
    px_same = same.all(axis=-1)
    n_diff = int((~px_same).sum())
    ulps = np.abs(dev.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))[~same]
    print(f"\n{w}x{h} f={f} k1={k1}: {n_diff} of {w * h} pixels with a differing map coordinate, max {int(ulps.max()) if ulps.size else 0} ulp")
    assert n_diff <= (w * h) * 1e-6
    assert not ulps.size or ulps.max() <= 1
    # the pixels are equal wherever the map is
    rng = np.random.default_rng(w * 7 + h)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    out = api.undistort(img, f, k1)
    href, _ = host.image(img, f, k1, threads=16)
    assert np.array_equal(out[px_same], href[px_same])


def _raw_scene(tiny_scene, k1s):
    views = [dataclasses.replace(v, k1=k) for v, k in zip(tiny_scene.views, k1s)]
    return dataclasses.replace(tiny_scene, views=views)


def _host_undistorted_scene(tiny_scene, k1s, host):
    views = []
    for v, k in zip(tiny_scene.views, k1s):
        out, _ = host.image(v.rgb, np.float32(v.f), k, threads=16)
        views.append(dataclasses.replace(v, rgb=out, k1=0.0))
    return dataclasses.replace(tiny_scene, views=views)


def test_scene_with_raw_views_equals_host_undistorted_scene(api, host, tiny_scene, tiny_seeds):
    k1s = [0.08, -0.12, -0.6][: tiny_scene.n_views] + [0.02] * max(0, tiny_scene.n_views - 3)
    raw = api.Scene(_raw_scene(tiny_scene, k1s), device=0)
    pre = api.Scene(_host_undistorted_scene(tiny_scene, k1s, host), device=0)
    try:
        la, lb = _levels(raw, tiny_scene.n_views), _levels(pre, tiny_scene.n_views)
        for i, (a, b) in enumerate(zip(la, lb)):
            assert len(a) == len(b)
            for l, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(x, y), f"view {i} level {l}"
        # the raw level 0 really was resampled
        assert not np.array_equal(la[0][0], np.ascontiguousarray(tiny_scene.views[0].rgb))
        ba = api.optimize_batch(raw, api.Batch.from_seeds(tiny_seeds))
        bb = api.optimize_batch(pre, api.Batch.from_seeds(tiny_seeds))
        assert int(ba.ok.sum()) > 0
        for name in api.Batch.FIELDS:
            x, y = getattr(ba, name, None), getattr(bb, name, None)
            if x is None:
                continue
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    finally:
        raw.close()
        pre.close()


def _write_nvm(path, scene, k1s, xyz, off, img):
    with open(path, "w") as f:
        f.write("NVM_V3\n\n%d\n" % scene.n_views)
        for i, v in enumerate(scene.views):
            f.write("view%02d.ppm %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g 0\n" %
                    (i, v.f, v.q[0], v.q[1], v.q[2], v.q[3], v.c[0], v.c[1], v.c[2], k1s[i]))
        f.write("\n%d\n" % len(xyz))
        for k in range(len(xyz)):
            ms = img[off[k]:off[k + 1]]
            f.write("%.17g %.17g %.17g 128 128 128 %d" % (xyz[k, 0], xyz[k, 1], xyz[k, 2], len(ms)))
            for m in ms:
                f.write(" %d %d 0 0" % (m, k))
            f.write("\n")
        f.write("\n0\n")


def _run_model(exe, d, scene, k1s, xyz, off, img):
    os.makedirs(d, exist_ok=True)
    for i, v in enumerate(scene.views):
        with open(os.path.join(d, "view%02d.ppm" % i), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (v.width, v.height) + np.ascontiguousarray(v.rgb).tobytes())
    _write_nvm(os.path.join(d, "scene.nvm"), scene, k1s, xyz, off, img)
    subprocess.run([exe, os.path.join(d, "scene.nvm"), os.path.join(d, "out.ply"), os.path.join(d, "copy.nvm"), "2"],
                   check=True, capture_output=True, text=True, timeout=600)
    return open(os.path.join(d, "out.ply"), "rb").read()


def test_cpp_nvm_model_with_radial_distortion(api, host, tiny_scene, tmp_path):
    """Scene::addCameras on an NVM model with r != 0 and raw PPMs: the PLY equals the one of the same model with r = 0
    and host-undistorted PPMs (Camera::init ignores r, so only the pixels differ)."""
    from hpmvs_amd import synth
    exe = os.path.join(ROOT, "tests", "native", "run_nvm_scene")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), "all"], check=True, capture_output=True)
    k1s = [float(np.float32(k)) for k in [0.05, -0.08, 0.15][: tiny_scene.n_views]] + [0.0] * max(0, tiny_scene.n_views - 3)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 300, start_level=2, noise=1.0)
    raw = _run_model(exe, str(tmp_path / "raw"), tiny_scene, k1s, xyz, off, img)
    pre = _run_model(exe, str(tmp_path / "pre"), _host_undistorted_scene(tiny_scene, k1s, host), [0.0] * tiny_scene.n_views,
                     xyz, off, img)
    plain = _run_model(exe, str(tmp_path / "plain"), tiny_scene, [0.0] * tiny_scene.n_views, xyz, off, img)
    assert raw == pre
    assert raw != plain   # the distortion changed what was reconstructed


def _bilinear(img, x, y):
    h, w = img.shape[:2]
    x = np.clip(x, 0, w - 1.001)
    y = np.clip(y, 0, h - 1.001)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    dx, dy = (x - x0)[..., None], (y - y0)[..., None]
    a, b = img[y0, x0], img[y0, x0 + 1]
    c, d = img[y0 + 1, x0], img[y0 + 1, x0 + 1]
    return (a * (1 - dx) + b * dx) * (1 - dy) + (c * (1 - dx) + d * dx) * dy


@pytest.mark.parametrize("k1", [0.15, -0.15])
def test_sign_convention_against_a_forward_distortion(api, k1):
    """D(p) = U(p (1 + k1 |p|^2)) in normalised coordinates; undistorting D must give back U (the reference samples the
    point m with m (1 + k1 |m|^2) = p).  Independent of the restatement: numpy forward model, device inverse."""
    w, h = 640, 480
    f = 1.1 * w
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    U = np.stack([128 + 100 * np.sin(xx / 37.0) * np.cos(yy / 29.0), 128 + 90 * np.sin((xx + yy) / 53.0),
                  128 + 80 * np.cos(xx / 41.0 - yy / 23.0)], axis=-1)
    px, py = (xx - w / 2.0) / f, (yy - h / 2.0) / f
    s = 1 + k1 * (px * px + py * py)
    D = _bilinear(U, px * s * f + w / 2.0, py * s * f + h / 2.0)
    D8 = np.clip(np.round(D), 0, 255).astype(np.uint8)
    U8 = np.clip(np.round(U), 0, 255).astype(np.uint8)
    inner = np.zeros((h, w), bool)
    inner[h // 6: -h // 6, w // 6: -w // 6] = True
    good = np.abs(api.undistort(D8, f, k1).astype(float) - U8)[inner].mean()
    wrong = np.abs(api.undistort(D8, f, -k1).astype(float) - U8)[inner].mean()
    print(f"\nk1={k1}: mean |undistort(D) - U| = {good:.3f} grey levels (opposite sign: {wrong:.3f})")
    # first MI355X run: 0.51 (k1 = 0.15) and 0.43 (k1 = -0.15) grey levels, the opposite sign 3.2
    assert good < 2.0
    assert wrong > 4 * good


def test_undistort_argument_errors(api, tiny_scene):
    L = api.lib()
    img = np.zeros((16, 16, 3), np.uint8)
    out = np.zeros_like(img)
    xy = np.zeros((16, 16, 2), np.float32)
    for f, k1 in [(0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.0), (20.0, float("nan")),
                  (20.0, float("inf"))]:
        assert L.hpmvs_undistort(0, img.ctypes.data, 16, 16, f, k1, out.ctypes.data, 0) == HPMVS_ERR_ARG
        assert L.hpmvs_undistort_map(0, 16, 16, f, k1, xy.ctypes.data) == HPMVS_ERR_ARG
    assert L.hpmvs_undistort(0, img.ctypes.data, 1, 16, 20.0, 0.1, out.ctypes.data, 0) == HPMVS_ERR_ARG
    assert L.hpmvs_undistort(99, img.ctypes.data, 16, 16, 20.0, 0.1, out.ctypes.data, 0) == HPMVS_ERR_ARG
    h = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(h)))
    try:
        v = tiny_scene.views[0]
        cam = api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, tiny_scene.max_level)
        rgb = np.ascontiguousarray(v.rgb)
        for f, k1 in [(0.0, 0.1), (float("nan"), 0.1), (v.f, float("inf")), (v.f, float("nan"))]:
            assert L.hpmvs_scene_set_view_distorted(h, 0, v.width, v.height, rgb.ctypes.data, 0, C.byref(cam), f, k1) == HPMVS_ERR_ARG
        assert L.hpmvs_scene_set_view_distorted(h, 1, v.width, v.height, rgb.ctypes.data, 0, C.byref(cam), v.f, 0.1) == HPMVS_ERR_ARG
        assert L.hpmvs_scene_set_view_distorted(h, 0, v.width, v.height, rgb.ctypes.data, 0, C.byref(cam), v.f, 0.1) == 0
    finally:
        L.hpmvs_scene_destroy(h)
