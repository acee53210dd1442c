#!/usr/bin/env python3
"""Baseline JPEG decoding of one view at production size (a 3840x2160 4:2:0 file by default): the host entropy stage on one
thread, the coefficient upload and the two kernels (hpmvs_jpeg_decode_timed: HIP events), the bytes the kernels must move
against the HBM peak, and hpmvs_scene_set_view_jpeg end to end against hpmvs_scene_set_view with already-decoded pixels
plus a full host decode of the same file (Pillow's when it imports, else the host restatement's, tests/jpeg_host.cpp).
Prints one JSON object and writes it to --out.

    python tools/jpeg_scale.py view.jpg [--out profiles/jpeg_scale.json]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, 8.0 TB/s (specification; a float4 copy reaches about 6.3 TB/s of it)


def stats(ts):
    return {"min": float(min(ts)), "median": float(np.median(ts))}


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("jpeg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_scale.json"))
    a = ap.parse_args()
    import torch
    from hpmvs_amd import api, synth
    from jpeg_ref import HostJpeg

    data = open(a.jpeg, "rb").read()
    w, h, comps, hs, vs = api.jpeg_info(data)
    L = api.lib()
    res = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "file_bytes": len(data), "w": w, "h": h,
           "components": comps, "h_samp": hs, "v_samp": vs, "reps": a.reps, "warmup": a.warmup}

    # stages of one decode to a device buffer
    out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
    ms = (C.c_float * 4)()
    rows = []
    for k in range(a.warmup + a.reps):
        api._chk(L.hpmvs_jpeg_decode_timed(0, data, len(data), out.data_ptr(), out.numel(), ms))
        if k >= a.warmup:
            rows.append(list(ms))
    rows = np.array(rows)
    for k, name in enumerate(["host_entropy_1_thread_ms", "coef_upload_ms", "idct_kernel_ms", "rgb_kernel_ms"]):
        res[name] = stats(rows[:, k])
    # what the kernels must move, from the shapes: coefficients read, planes written and read again, RGB written
    mcu_w, mcu_h = 8 * hs, 8 * vs
    mx, my = -(-w // mcu_w), -(-h // mcu_h)
    samples = mx * my * (64 * hs * vs + (128 if comps == 3 else 0))
    idct_bytes, rgb_bytes = 3 * samples, samples + 3 * w * h
    res["idct_bytes"], res["rgb_bytes"] = idct_bytes, rgb_bytes
    res["hbm_peak_gbs_MI355X_MICROARCH"] = HBM_PEAK_GBS
    res["idct_gbs"] = idct_bytes / (res["idct_kernel_ms"]["median"] * 1e6)
    res["rgb_gbs"] = rgb_bytes / (res["rgb_kernel_ms"]["median"] * 1e6)
    res["idct_fraction_of_hbm_peak"] = res["idct_gbs"] / HBM_PEAK_GBS
    res["rgb_fraction_of_hbm_peak"] = res["rgb_gbs"] / HBM_PEAK_GBS
    res["jpeg_decode_host_destination_ms"] = wall_ms(lambda: api.jpeg_decode(data), a.reps)

    # scene upload of the view: JPEG bytes against decoded pixels
    pixels = api.jpeg_decode(data)
    cam = synth.make_cameras(3, w, h)[0]
    hc = api.camera_from_nvm(cam.f, cam.q, cam.c, w, h, 5)
    sc = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(sc)))
    try:
        def set_jpeg():
            api._chk(L.hpmvs_scene_set_view_jpeg(sc, 0, data, len(data), C.byref(hc), float(cam.f), 0.0))

        def set_pixels():
            api._chk(L.hpmvs_scene_set_view(sc, 0, w, h, pixels.ctypes.data, 0, C.byref(hc)))
        for _ in range(a.warmup):
            set_jpeg()
            set_pixels()
        res["scene_set_view_jpeg_ms"] = wall_ms(set_jpeg, a.reps)
        res["scene_set_view_decoded_pixels_ms"] = wall_ms(set_pixels, a.reps)
    finally:
        L.hpmvs_scene_destroy(sc)
    try:
        from PIL import Image
        res["full_host_decode"] = "Pillow"
        res["full_host_decode_ms"] = wall_ms(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), 5)
    except ImportError:
        with tempfile.TemporaryDirectory() as tmp:
            H = HostJpeg(tmp)
            res["full_host_decode"] = "host restatement (tests/jpeg_host.cpp, one thread)"
            res["full_host_decode_ms"] = wall_ms(lambda: H.decode(data, w, h), 5)
    res["host_decode_plus_set_view_ms"] = res["full_host_decode_ms"]["median"] + res["scene_set_view_decoded_pixels_ms"]["median"]
    with tempfile.TemporaryDirectory() as tmp:
        rc, ref, _ = HostJpeg(tmp).decode(data, w, h)
    res["device_equals_host_restatement"] = bool(rc == 0 and np.array_equal(ref, pixels))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
