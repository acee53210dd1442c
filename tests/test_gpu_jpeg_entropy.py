"""The JPEG scan's Huffman data decoded on the GPU (kernel_jpeg_entropy.hip) against the host walk, decode_file, which
tests/test_cpu_jpeg.py pins to libjpeg: every coefficient of the 20 fixture files at every subsequence size with the host
restatement's round count, Pillow's pixels through the device decode, seeded mutations (what the device takes is the host's,
what it does not take is exactly what the restatement leaves to the host), a scene, and the argument errors."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from jpeg_entropy_ref import DEVICE, HOST, SHIPPED_BITS, SWEEP, EntropyHost, files, mutation_set
from jpeg_ref import GUARD, Golden

pytestmark = pytest.mark.gpu
AUTO, ERR_ARG, ERR_STATE = 0, -2, -3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return EntropyHost(tmp_path_factory.mktemp("jpeg_entropy_host"))


@pytest.fixture(scope="module")
def golden():
    return Golden()


@pytest.fixture(scope="module")
def api():
    from hpmvs_amd import api as a
    if a.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    return a


def _coefficients(api, data, entropy, bits, n):
    """hpmvs_jpeg_coefficients into a fenced buffer of n elements -> (code, message, coefficients, used, rounds)"""
    raw = np.full(2 * GUARD + max(n, 1), 0x5A5A, np.int16)
    used, rounds = C.c_int(-1), C.c_int(-1)
    rc = api.lib().hpmvs_jpeg_coefficients(0, data, len(data), entropy, bits, raw.ctypes.data + 2 * GUARD, n, C.byref(used), C.byref(rounds))
    assert (raw[:GUARD] == 0x5A5A).all() and (raw[GUARD + max(n, 1):] == 0x5A5A).all(), "a guard element was written"
    msg = api.lib().hpmvs_last_error().decode() if rc else ""
    return rc, msg, raw[GUARD:GUARD + n].copy(), used.value, rounds.value


def test_device_coefficients_equal_the_hosts_at_every_subsequence_size(api, host):
    for name, data in files():
        n = host.L.je_n_coef(data, len(data))
        rc, _, truth, used, _ = _coefficients(api, data, HOST, 0, n)
        assert rc == 0 and used == HOST and np.array_equal(truth, host.host(data)[1]), name
        for bits in SWEEP:
            rc, msg, coef, used, rounds = _coefficients(api, data, DEVICE, bits if bits != SHIPPED_BITS else 0, n)
            assert rc == 0, (name, bits, msg)
            assert used == DEVICE, (name, bits)
            assert np.array_equal(coef, truth), f"{name} at {bits} bits: {int((coef != truth).sum())} coefficients differ"
            assert rounds == host.scheme(data, bits)[4], (name, bits)
    name, data = files()[0]                          # no upper bound on the size: every segment is one subsequence
    n = host.L.je_n_coef(data, len(data))
    rc, msg, coef, used, rounds = _coefficients(api, data, DEVICE, 1 << 30, n)
    assert (rc, used, rounds) == (0, DEVICE, 0) and np.array_equal(coef, host.host(data)[1]), msg


def test_pixels_through_the_device_decode_equal_pillows(api, golden):
    import torch
    L = api.lib()
    for n in golden.names:
        w, h = golden.info[n][:2]
        data = golden.jpg[n]
        used = C.c_int(-1)
        raw = np.full(2 * GUARD + 3 * w * h, 0xA5, np.uint8)
        api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), raw.ctypes.data + GUARD, 3 * w * h, 0, DEVICE, C.byref(used)))
        assert used.value == DEVICE, n
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), n
        assert np.array_equal(raw[GUARD:-GUARD].reshape(h, w, 3), golden.rgb[n]), n
        dev = torch.full((2 * GUARD + 3 * w * h,), 0xA5, dtype=torch.uint8, device="cuda:0")
        api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), dev.data_ptr() + GUARD, 3 * w * h, 1, DEVICE, None))
        dev = dev.cpu().numpy()
        assert (dev[:GUARD] == 0xA5).all() and (dev[-GUARD:] == 0xA5).all(), n
        assert np.array_equal(dev[GUARD:-GUARD].reshape(h, w, 3), golden.rgb[n]), n
    assert np.array_equal(api.jpeg_decode(golden.jpg[golden.names[0]], entropy="device"), golden.rgb[golden.names[0]])


def test_mutations_auto_is_the_host_and_device_refuses_what_the_restatement_leaves_to_the_host(api, host):
    taken = refused = 0
    for name, k, m in mutation_set():
        n = host.L.je_n_coef(m, len(m))
        rc_h, msg_h, truth, _, _ = _coefficients(api, m, HOST, 0, n)
        rc_a, msg_a, coef_a, _, _ = _coefficients(api, m, AUTO, 0, n)
        assert (rc_a, msg_a) == (rc_h, msg_h), (name, k)
        assert rc_h != 0 or np.array_equal(coef_a, truth), (name, k)
        rc_d, msg_d, coef_d, used, _ = _coefficients(api, m, DEVICE, 0, n)
        if n == 0:                                   # the headers are refused: the file's own code and message
            assert (rc_d, msg_d) == (rc_h, msg_h), (name, k)
        elif host.scheme(m)[3]:                      # the restatement accepts the parallel decode
            assert rc_h == 0 and rc_d == 0 and used == DEVICE and np.array_equal(coef_d, truth), (name, k)
            taken += 1
        else:
            assert rc_d == ERR_STATE and msg_d.startswith("jpeg: "), (name, k, rc_d, msg_d)
            refused += 1
    print(f"\n{taken} mutations decoded on the device, {refused} refused by it")
    assert taken >= 400 and refused >= 100


def test_auto_takes_the_device_from_its_threshold_on_and_the_pixels_do_not_change(api, golden):
    """_AUTO measures the file from its scan's first byte on: bytes behind EOI, which every decoder here ignores, lift a small
    file over the threshold"""
    import os
    import re
    L = api.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hpmvs_amd.h")).read()
    threshold = int(re.search(r"#define HPMVS_JPEG_AUTO_MIN_SCAN_BYTES (\d+)", header).group(1))
    name = "c200x136_420_q85"
    w, h = golden.info[name][:2]
    assert len(golden.jpg[name]) < threshold
    for data, want in ((golden.jpg[name], HOST), (golden.jpg[name] + bytes(threshold), DEVICE)):
        used = C.c_int(-1)
        out = np.zeros((h, w, 3), np.uint8)
        api._chk(L.hpmvs_jpeg_decode_ex(0, data, len(data), out.ctypes.data, out.nbytes, 0, AUTO, C.byref(used)))
        assert used.value == want and np.array_equal(out, golden.rgb[name])


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


def test_scene_with_scans_decoded_on_the_device_equals_the_host_one(api, golden, tiny_scene):
    """every level of every view; view 0 with k1 != 0"""
    assert tiny_scene.n_views == len(golden.scene_jpg)
    views = [dataclasses.replace(v, rgb=b, k1=k) for v, b, k in zip(tiny_scene.views, golden.scene_jpg, [0.05, 0.0, 0.0])]
    sc = dataclasses.replace(tiny_scene, views=views)
    a = api.Scene(sc, device=0, jpeg_entropy="device")
    b = api.Scene(sc, device=0, jpeg_entropy="host")
    try:
        la, lb = _levels(a, sc.n_views), _levels(b, sc.n_views)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert len(x) == len(y) >= 2
            for l, (p, q) in enumerate(zip(x, y)):
                assert np.array_equal(p, q), f"view {i} level {l}"
        assert np.array_equal(la[2][0], api.jpeg_decode(golden.scene_jpg[2], entropy="host"))
    finally:
        a.close()
        b.close()
    used = C.c_int(-1)
    h = C.c_void_p()
    v = tiny_scene.views[0]
    api._chk(api.lib().hpmvs_scene_create(1, 0, C.byref(h)))
    try:
        cam = api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, tiny_scene.max_level)
        good = golden.scene_jpg[0]
        api._chk(api.lib().hpmvs_scene_set_view_jpeg_ex(h, 0, good, len(good), C.byref(cam), float(v.f), 0.0, DEVICE, C.byref(used)))
        assert used.value == DEVICE
        assert api.lib().hpmvs_scene_set_view_jpeg_ex(h, 0, good, len(good), C.byref(cam), float(v.f), 0.0, 3, None) == ERR_ARG
    finally:
        api.lib().hpmvs_scene_destroy(h)


def test_argument_errors_come_before_any_write(api, host):
    name, data = files()[0]
    n = host.L.je_n_coef(data, len(data))
    for entropy, bits, cap in ((3, 0, n), (-1, 0, n), (DEVICE, 48, n), (DEVICE, 32, n), (DEVICE, 100, n), (DEVICE, -64, n), (HOST, 0, n - 1),
                               (DEVICE, 0, n - 1)):
        raw = np.full(n + GUARD, 0x5A5A, np.int16)
        used, rounds = C.c_int(-7), C.c_int(-7)
        rc = api.lib().hpmvs_jpeg_coefficients(0, data, len(data), entropy, bits, raw.ctypes.data, cap, C.byref(used), C.byref(rounds))
        assert rc == ERR_ARG, (entropy, bits, cap, rc)
        assert (raw == 0x5A5A).all() and used.value == -7 and rounds.value == -7, (entropy, bits, cap)
    out = np.full(3 * 96 * 64 + GUARD, 0xA5, np.uint8)
    assert api.lib().hpmvs_jpeg_decode_ex(0, data, len(data), out.ctypes.data, 3 * 96 * 64, 0, 7, None) == ERR_ARG
    assert api.lib().hpmvs_jpeg_decode_ex(0, data, len(data), out.ctypes.data, 3 * 96 * 64 - 1, 0, DEVICE, None) == ERR_ARG
    assert (out == 0xA5).all()
    with pytest.raises(api.HpmvsError):
        api.jpeg_decode(data, entropy="gpu")


# ---- the fallback: the device tries, the prescan or the check refuses, the host walk takes over
def _threshold():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hpmvs_amd.h")).read()
    return int(re.search(r"#define HPMVS_JPEG_AUTO_MIN_SCAN_BYTES (\d+)", header).group(1))


def test_mutations_over_the_threshold_auto_tries_the_device_and_falls_back_to_the_host(api, host):
    """every mutation with bytes behind it that lift it over _AUTO's threshold: code, message and coefficients are _HOST's on
    the same bytes, and the host walk ran exactly where the restatement leaves the file to it"""
    pad = bytes(_threshold())
    on_device = fell_back = refused_by_both = 0
    for name, k, m in mutation_set():
        p = m + pad
        n = host.L.je_n_coef(p, len(p))
        rc_h, msg_h, truth, used_h, _ = _coefficients(api, p, HOST, 0, n)
        rc_a, msg_a, coef_a, used_a, rounds_a = _coefficients(api, p, AUTO, 0, n)
        assert (rc_a, msg_a) == (rc_h, msg_h), (name, k)
        if rc_h != 0:
            refused_by_both += n > 0
            continue
        assert used_h == HOST and np.array_equal(coef_a, truth), (name, k)
        _, _, _, accepted, rounds = host.scheme(p)
        assert used_a == (DEVICE if accepted else HOST), (name, k)
        assert rounds_a == (rounds if accepted else 0), (name, k)
        on_device += accepted
        fell_back += not accepted
    print(f"\n_AUTO over the threshold: {on_device} decoded on the device, {fell_back} fell back to the host walk, "
          f"{refused_by_both} refused by the host walk behind the device's attempt")
    assert on_device >= 400 and fell_back >= 50 and refused_by_both >= 100


@pytest.fixture(scope="module")
def refused(api, host, golden):
    """two files the host accepts and the device does not take, made from the scene's first view: FF FF fill in the scan (the
    prescan refuses it), and the first seeded mutation whose chain the check kernel refuses"""
    from jpeg_ref import mutations
    view = golden.scene_jpg[0]
    assert view[-2:] == b"\xff\xd9"
    out = {"fill": view[:-2] + b"\xff" + view[-2:]}
    for m in mutations(view, seed=0, n_overwrites=400, n_cuts=0):
        n = host.L.je_n_coef(m, len(m))
        if n == 0 or host.host(m)[0] != 0 or api.jpeg_info(m)[:2] != api.jpeg_info(view)[:2]:
            continue
        rc, msg, _, _, _ = _coefficients(api, m, DEVICE, 0, n)
        if rc == ERR_STATE and "check refused" in msg:
            out["chain"] = m
            break
    assert "chain" in out
    rc, msg, _, _, _ = _coefficients(api, out["fill"], DEVICE, 0, host.L.je_n_coef(out["fill"], len(out["fill"])))
    assert rc == ERR_STATE and "fill bytes" in msg
    return out


def _pixels(api, data, w, h, entropy):
    raw = np.full(2 * GUARD + 3 * w * h, 0xA5, np.uint8)
    used = C.c_int(-1)
    api._chk(api.lib().hpmvs_jpeg_decode_ex(0, data, len(data), raw.ctypes.data + GUARD, 3 * w * h, 0, entropy, C.byref(used)))
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    return raw[GUARD:-GUARD].reshape(h, w, 3).copy(), used.value


@pytest.mark.parametrize("which", ["fill", "chain"])
def test_pixels_and_a_scene_view_behind_a_refused_device_decode_are_the_hosts(api, golden, tiny_scene, refused, which):
    L = api.lib()
    w, h = golden.scene_size
    data = refused[which]
    padded = data + bytes(_threshold())
    truth, used = _pixels(api, data, w, h, HOST)
    assert used == HOST
    if which == "fill":
        assert np.array_equal(truth, api.jpeg_decode(golden.scene_jpg[0], entropy="host"))   # fill bytes change no pixel
    got, used = _pixels(api, padded, w, h, AUTO)
    assert used == HOST and np.array_equal(got, truth)
    v = tiny_scene.views[0]
    sc = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(sc)))
    try:
        cam = api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, tiny_scene.max_level)
        assert L.hpmvs_scene_set_view_jpeg_ex(sc, 0, padded, len(padded), C.byref(cam), float(v.f), 0.0, DEVICE, None) == ERR_STATE
        used = C.c_int(-1)
        api._chk(L.hpmvs_scene_set_view_jpeg_ex(sc, 0, padded, len(padded), C.byref(cam), float(v.f), 0.0, AUTO, C.byref(used)))
        assert used.value == HOST
        api._chk(L.hpmvs_scene_commit(sc))
        ww, hh = C.c_int(), C.c_int()
        lvl = np.empty((h, w, 3), np.uint8)
        api._chk(L.hpmvs_scene_get_level(sc, 0, 0, lvl.ctypes.data, lvl.nbytes, C.byref(ww), C.byref(hh)))
        assert (ww.value, hh.value) == (w, h) and np.array_equal(lvl, truth)
    finally:
        L.hpmvs_scene_destroy(sc)


def test_environment_names_the_mode_of_the_existing_entries(api, golden, refused):
    """HPMVS_JPEG_ENTROPY is read once per process, so two processes of their own, side by side.  `device`: the existing entry
    decodes a small intact file on the GPU (which _AUTO would leave to the host) and the two refused files through the host
    walk.  `host`: it decodes on the host a file over _AUTO's threshold.  hpmvs_jpeg_last_decode tells what ran; the pixels
    are the host's everywhere."""
    import hashlib
    import os
    import subprocess
    import sys
    import tempfile
    w, h = golden.scene_size
    cases = [golden.scene_jpg[0], refused["fill"], refused["chain"], golden.scene_jpg[0] + bytes(_threshold())]
    want = [hashlib.sha256(_pixels(api, d, w, h, HOST)[0].tobytes()).hexdigest() for d in cases]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C, hashlib, sys; sys.path.insert(0, %r); from hpmvs_amd import api\n"
            "for p in sys.argv[1:]:\n"
            "    px = api.jpeg_decode(open(p, 'rb').read()); used = C.c_int(-1)\n"
            "    api._chk(api.lib().hpmvs_jpeg_last_decode(C.byref(used), None))\n"
            "    print(used.value, hashlib.sha256(px.tobytes()).hexdigest())\n" % root)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, d in enumerate(cases):
            paths.append(os.path.join(tmp, f"{i}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(d)
        procs = {mode: subprocess.Popen([sys.executable, "-c", code] + paths, env=dict(os.environ, HPMVS_JPEG_ENTROPY=mode),
                                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for mode in ("device", "host", "auto")}
        outs = {}
        for mode, p in procs.items():
            out, err = p.communicate(timeout=120)
            assert p.returncode == 0, (mode, err[-2000:])
            outs[mode] = [ln.split() for ln in out.strip().splitlines()[-len(cases):]]
    for mode, used in (("device", [DEVICE, HOST, HOST, DEVICE]), ("host", [HOST] * 4), ("auto", [HOST, HOST, HOST, DEVICE])):
        assert [int(u) for u, _ in outs[mode]] == used, mode
        assert [hx for _, hx in outs[mode]] == want, mode
