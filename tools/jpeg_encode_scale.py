#!/usr/bin/env python3
"""Baseline JPEG encoding of one view at production size (a rendered 3840x2160 view by default) at quality 100 and 90: the
stages of one encode from a device buffer (hpmvs_jpeg_encode_timed: HIP events), hpmvs_scene_get_level_jpeg end to end (the
level encoded where it lies; wall clock, median of repeated calls after warm-up), and what it replaces: hpmvs_scene_get_level
plus a host encode of the pixels on one thread (Pillow's when it imports -- the comparison the figures in DESIGN.md 3.13b are
for -- else the host restatement's, tests/jpeg_enc_host.cpp).  Also checks the device's file against that host encode byte
for byte.  Prints one JSON object and writes it to --out.

    python tools/jpeg_encode_scale.py [--width 3840 --height 2160] [--out profiles/jpeg_encode_scale.json]
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
STAGES = ["first_buffer_and_tables_ms", "coef_kernel_ms", "lengths_scan_readback_ms", "second_buffer_and_fills_ms", "write_kernel_ms",
          "ff_count_scan_readback_ms", "stuff_kernel_ms", "copy_to_host_ms"]


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
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_scale.json"))
    a = ap.parse_args()
    import torch
    from hpmvs_amd import api, synth

    w, h = a.width, a.height
    scene = synth.make_scene(3, w, h, n_waves=24, device="cuda:0")
    view = scene.views[0]
    pixels_dev = view.rgb.contiguous()
    pixels = pixels_dev.cpu().numpy()
    L = api.lib()
    res = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "w": w, "h": h, "raw_bytes": int(pixels.nbytes),
           "reps": a.reps, "warmup": a.warmup, "quality": {}}
    try:
        import PIL
        from PIL import Image, features
        res["host_encoder"] = "Pillow %s over libjpeg %s" % (PIL.__version__, features.version("jpg"))

        def host_encode(px, q):
            f = io.BytesIO()
            Image.fromarray(px).save(f, "JPEG", quality=q, subsampling=2, optimize=False)
            return f.getvalue()
    except ImportError:
        from jpeg_enc_ref import HostJpegEnc
        H = HostJpegEnc(tempfile.mkdtemp())
        res["host_encoder"] = "host restatement (tests/jpeg_enc_host.cpp, one thread)"

        def host_encode(px, q):
            return H.encode(px, q)[1]

    hc = api.camera_from_nvm(view.f, view.q, view.c, w, h, 5)
    sc = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(sc)))
    try:
        api._chk(L.hpmvs_scene_set_view(sc, 0, w, h, pixels_dev.data_ptr(), 1, C.byref(hc)))
        out = np.empty(api.jpeg_encode_bound(w, h), np.uint8)
        lvl = np.empty((h, w, 3), np.uint8)
        n = C.c_size_t(0)
        ww, hh = C.c_int(), C.c_int()
        for q in (100, 90):
            r = {}
            ms = (C.c_float * 8)()
            rows = []
            for k in range(a.warmup + a.reps):
                api._chk(L.hpmvs_jpeg_encode_timed(0, pixels_dev.data_ptr(), w, h, q, out.ctypes.data, out.nbytes, C.byref(n), ms))
                if k >= a.warmup:
                    rows.append(list(ms))
            rows = np.array(rows)
            for k, name in enumerate(STAGES):
                r[name] = stats(rows[:, k])
            r["stages_sum_ms"] = float(sum(r[name]["median"] for name in STAGES))
            r["file_bytes"] = int(n.value)
            device_file = out[:n.value].tobytes()

            def level_jpeg():
                api._chk(L.hpmvs_scene_get_level_jpeg(sc, 0, 0, q, out.ctypes.data, out.nbytes, C.byref(n)))

            def level_then_host():
                api._chk(L.hpmvs_scene_get_level(sc, 0, 0, lvl.ctypes.data, lvl.nbytes, C.byref(ww), C.byref(hh)))
                return host_encode(lvl, q)

            def level_only():
                api._chk(L.hpmvs_scene_get_level(sc, 0, 0, lvl.ctypes.data, lvl.nbytes, C.byref(ww), C.byref(hh)))
            for _ in range(a.warmup):
                level_jpeg()
                level_then_host()
            # alternating, so that what else runs on the host falls on both alike
            t_dev, t_host, t_copy = [], [], []
            for _ in range(a.reps):
                t_dev.append(wall_ms(level_jpeg, 1)["min"])
                t_host.append(wall_ms(level_then_host, 1)["min"])
                t_copy.append(wall_ms(level_only, 1)["min"])
            r["scene_get_level_jpeg_ms"] = stats(t_dev)
            r["scene_get_level_plus_host_encode_ms"] = stats(t_host)
            r["scene_get_level_ms"] = stats(t_copy)
            r["device_faster_end_to_end"] = bool(r["scene_get_level_jpeg_ms"]["median"] < r["scene_get_level_plus_host_encode_ms"]["median"])
            r["device_file_equals_host_encode"] = bool(out[:n.value].tobytes() == device_file == level_then_host())
            res["quality"][str(q)] = r
    finally:
        L.hpmvs_scene_destroy(sc)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
