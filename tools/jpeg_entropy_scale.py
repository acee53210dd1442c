#!/usr/bin/env python3
"""The JPEG scan's entropy decode on the GPU (kernel_jpeg_entropy.hip) against the host walk, per file: the stages of one
device decode (hpmvs_jpeg_entropy_timed: prescan by wall clock, every kernel and the uploads by HIP events) and
hpmvs_scene_set_view_jpeg_ex end to end with _HOST and _DEVICE alternating in one loop, as medians of --reps after
--warmup; with --parent-lib the same end to end figure from another build of the library (the parent commit's, built
into tools/ab/parent/), taken in a child process that loads it through HPMVS_LIB.  Writes one JSON object with the
threshold the figures give for _AUTO: the smallest scan from which _DEVICE beats the parent by more than the box-to-box
spread.  --kernel-stats takes the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv` run of its
own over `--trace-only FILE.jpg` (four device decodes of the file and nothing else) into the record.

    python tools/jpeg_entropy_scale.py --make-inputs DIR        # development machine, needs Pillow: seeded synth views
    python tools/jpeg_entropy_scale.py DIR/*.jpg [--parent-lib tools/ab/parent/libhpmvs_amd.so] [--kernel-stats CSV]
                                       [--out profiles/jpeg_entropy_scale.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPREAD = 0.015   # box-to-box spread of a wall-clock median on these machines (Measuring)
STAGES = ["prescan_ms", "scan_upload_and_fills_ms", "sync_kernel_all_passes_ms", "sync_passes_with_readbacks_ms", "scan_local_kernel_ms",
          "scan_groups_kernel_ms", "check_kernel_ms", "write_kernel_ms", "quantiser_upload_ms", "idct_kernel_ms", "rgb_kernel_ms", "rounds"]


def make_inputs(out_dir):
    from PIL import Image
    from hpmvs_amd import synth
    os.makedirs(out_dir, exist_ok=True)
    for w, h in ((640, 480), (1920, 1080), (3840, 2160)):
        view = synth.make_scene(1, w, h).views[0]
        img = Image.fromarray(np.ascontiguousarray(view.rgb))
        for q in (50, 90):
            img.save(os.path.join(out_dir, f"synth_{w}x{h}_q{q}.jpg"), "JPEG", quality=q, subsampling=2)
        if w == 3840:
            img.save(os.path.join(out_dir, f"synth_{w}x{h}_q90_rstrow.jpg"), "JPEG", quality=90, subsampling=2, restart_marker_rows=1)


def scan_bytes(data):
    i = 2
    while True:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        i += 2 + ln
        if m == 0xDA:
            return len(data) - i


def end_to_end(api, data, modes, reps, warmup):
    """hpmvs_scene_set_view_jpeg(_ex) wall clock per mode, the modes alternating -> {mode: median ms}"""
    from hpmvs_amd import synth
    L = api.lib()
    w, h = api.jpeg_info(data)[:2]
    cam = synth.make_cameras(3, w, h)[0]
    hc = api.camera_from_nvm(cam.f, cam.q, cam.c, w, h, 5)
    sc = C.c_void_p()
    api._chk(L.hpmvs_scene_create(1, 0, C.byref(sc)))
    ts = {m: [] for m in modes}
    try:
        for k in range(warmup + reps):
            for m in modes:
                t = time.perf_counter()
                if m is None:
                    api._chk(L.hpmvs_scene_set_view_jpeg(sc, 0, data, len(data), C.byref(hc), float(cam.f), 0.0))
                else:
                    api._chk(L.hpmvs_scene_set_view_jpeg_ex(sc, 0, data, len(data), C.byref(hc), float(cam.f), 0.0, api.JPEG_ENTROPY[m], None))
                if k >= warmup:
                    ts[m].append(1e3 * (time.perf_counter() - t))
    finally:
        L.hpmvs_scene_destroy(sc)
    return {str(m): float(np.median(v)) for m, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("jpegs", nargs="*")
    ap.add_argument("--make-inputs")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--child", action="store_true", help="(internal) print the end-to-end medians of the loaded library and leave")
    ap.add_argument("--trace-only", help="decode this file four times on the device and leave (the program of a rocprofv3 run)")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of that rocprofv3 run, taken into the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_entropy_scale.json"))
    a = ap.parse_args()
    if a.make_inputs:
        return make_inputs(a.make_inputs)
    from hpmvs_amd import api
    if a.trace_only:
        data = open(a.trace_only, "rb").read()
        for _ in range(4):
            api.jpeg_decode(data, on_device=True, entropy="device")
        return
    if a.child:
        # another build of the library, which need not have the newer entries: only what end_to_end calls is declared
        L = C.CDLL(os.environ["HPMVS_LIB"])
        L.hpmvs_last_error.restype = C.c_char_p
        L.hpmvs_camera_from_nvm.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                                            C.POINTER(api.Camera)]
        L.hpmvs_scene_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.hpmvs_scene_destroy.argtypes = [C.c_void_p]
        L.hpmvs_jpeg_info.argtypes = [C.c_char_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5
        L.hpmvs_scene_set_view_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(api.Camera), C.c_float, C.c_float]
        api._lib = L
        print(json.dumps({os.path.basename(p): end_to_end(api, open(p, "rb").read(), [None], a.reps, a.warmup)["None"] for p in a.jpegs}))
        return
    import torch
    L = api.lib()
    parent = {}
    if a.parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)] + a.jpegs,
                           env=dict(os.environ, HPMVS_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, check=True,
                           timeout=900)
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    res = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "spread": SPREAD,
           "parent_lib": a.parent_lib, "files": []}
    for p in sorted(a.jpegs, key=os.path.getsize):
        data = open(p, "rb").read()
        w, h = api.jpeg_info(data)[:2]
        row = {"file": os.path.basename(p), "w": w, "h": h, "file_bytes": len(data), "scan_bytes": scan_bytes(data)}
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
        ms = (C.c_float * len(STAGES))()
        rows = []
        for k in range(a.warmup + a.reps):
            api._chk(L.hpmvs_jpeg_entropy_timed(0, data, len(data), out.data_ptr(), out.numel(), ms))
            if k >= a.warmup:
                rows.append(list(ms))
        for k, name in enumerate(STAGES):
            row[name] = float(np.median(np.array(rows)[:, k]))
        row["device_pixels_equal_host"] = bool(np.array_equal(out.cpu().numpy(), api.jpeg_decode(data, entropy="host")))
        e2e = end_to_end(api, data, ["host", "device"], a.reps, a.warmup)
        row["set_view_host_ms"], row["set_view_device_ms"] = e2e["host"], e2e["device"]
        if parent:
            row["set_view_parent_ms"] = parent[os.path.basename(p)]
            row["device_beats_parent"] = bool(row["set_view_device_ms"] < (1.0 - SPREAD) * row["set_view_parent_ms"])
        res["files"].append(row)
    if parent:
        # the smallest scan from which _DEVICE wins, and goes on winning at every larger one
        wins = [r["device_beats_parent"] for r in res["files"]]
        first = next((k for k in range(len(wins)) if all(wins[k:])), None)
        largest = res["files"][-1]
        res["auto_min_scan_bytes"] = None if first is None or not largest["device_beats_parent"] else res["files"][first]["scan_bytes"]
    if a.kernel_stats:
        import csv
        with open(a.kernel_stats, newline="") as fh:
            res["rocprofv3_kernel_stats_of_4_decodes_of_the_largest_q90_file"] = [
                {"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": int(r["MinNs"]),
                 "max_ns": int(r["MaxNs"])} for r in csv.DictReader(fh)]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
