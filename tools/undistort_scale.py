#!/usr/bin/env python3
"""Level-0 undistortion at production size: the kernel (hpmvs_undistort on device pointers, host pointers end to end),
the scene upload of a 50-view 4K set through hpmvs_scene_set_view_distorted against hpmvs_scene_set_view, and the host
restatement (tests/undistort_host.cpp: the reference's per-pixel loop, same arithmetic) on 1 and 16 CPU threads.
Prints one JSON object and writes it to --out.

    python tools/undistort_scale.py [--views 50] [--out profiles/undistort_scale.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--k1", type=float, default=-0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hpmvs_amd import api, synth
    from undistort_ref import HostUndistort

    w, h, k1 = a.w, a.h, a.k1
    f = float(np.float32(1.2 * w))
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    res = {"build_id": api.build_id(), "w": w, "h": h, "f": f, "k1": k1, "views": a.views,
           "device": torch.cuda.get_device_name(0)}

    # one view, device pointers: kernel time from events around the call (the call synchronises)
    src = torch.from_numpy(img).to("cuda:0")
    dst = torch.empty_like(src)
    L = api.lib()
    for kk in (k1, -k1):
        api._chk(L.hpmvs_undistort(0, src.data_ptr(), w, h, f, kk, dst.data_ptr(), 1))  # warm-up
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.reps):
            ev0.record()
            api._chk(L.hpmvs_undistort(0, src.data_ptr(), w, h, f, kk, dst.data_ptr(), 1))
            ev1.record()
            ev1.synchronize()
            ms.append(ev0.elapsed_time(ev1))
        res[f"undistort_device_k1_{kk:+g}_ms"] = {"min": min(ms), "median": float(np.median(ms))}
    res["undistort_host_pointers_ms"] = wall(lambda: api.undistort(img, f, k1), a.reps)

    # scene upload, a views-strong set of 4K views (one shared pixel array), with and without k1
    cams = synth.make_cameras(a.views, w, h)
    covis = [[j for j in range(a.views) if j != i][:8] for i in range(a.views)]

    def upload(kk):
        views = [synth.View(v.width, v.height, v.f, v.q, v.c, img, kk) for v in cams]
        sc = api.Scene(synth.SynthScene(views, covis, max_level=5), device=0)
        sc.close()
    upload(0.0)
    res["scene_set_view_ms"] = wall(lambda: upload(0.0), 3)
    res["scene_set_view_distorted_ms"] = wall(lambda: upload(k1), 3)

    # host restatement (the reference's loop, one thread; and split over 16)
    with tempfile.TemporaryDirectory() as tmp:
        H = HostUndistort(tmp)
        res["host_1_thread_ms"] = wall(lambda: H.image(img, f, k1, threads=1), 2)
        res["host_16_threads_ms"] = wall(lambda: H.image(img, f, k1, threads=16), 3)
        ref, _ = H.image(img, f, k1, threads=16)
    res["device_equals_host_pixels"] = float((api.undistort(img, f, k1) == ref).all(-1).mean())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
