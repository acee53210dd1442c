#!/usr/bin/env python3
"""The patch cloud as an extended PLY file at production size: n synthetic patches with 8 image ids each (default n = 1e5 and
1e6), ASCII and binary, all fields.  One side is hpmvs_ply_ext_timed -- the stage times by HIP events (staging in, ply_len_kernel,
the scan and the total's read-back, ply_vertex_kernel, ply_list_kernel, the copy to the host) and the wall clock of the
host-pointer call, and of api.ply_ext, which makes a size query first and so converts, scans and stages twice.  The other side is the unchanged host mo3d::writeExtPly (tests/native/bench_ply_ext_host.cpp, built here with
g++) writing the same patches to /dev/shm in the same run: the only way to make the file without this entry.  Both files are
compared byte for byte.  The write kernels' achieved bytes per second stand beside a plain device-to-device copy of the same byte
count, the ceiling.  Medians of repeated calls after warm-up; no threshold rests on the numbers.  Prints one JSON object and
writes it to --out.

    python tools/ply_ext_scale.py [--sizes 100000 1000000] [--out profiles/ply_ext_scale.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("stage_in_ms", "len_kernel_ms", "scan_readback_ms", "vertex_kernel_ms", "list_kernel_ms", "copy_out_ms")


def med(ts):
    return {"min": float(min(ts)), "median": float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--ids", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_ext_scale.json"))
    a = ap.parse_args()
    import torch
    from hpmvs_amd import api

    if api.device_count() < 1:
        raise SystemExit("ply_ext_scale: no HIP device (there is no CPU path to measure)")
    shm = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    bin_dir = tempfile.mkdtemp()   # (/dev/shm may be mounted noexec)
    exe = os.path.join(bin_dir, "bench_ply_ext_host")
    lib = os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "bench_ply_ext_host.cpp"),
                    "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True)
    L = api.lib()
    res = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "ids_per_patch": a.ids, "reps": a.reps,
           "host_reps": a.host_reps, "warmup": a.warmup, "host_file_system": os.path.dirname(shm), "runs": []}
    for n in a.sizes:
        rng = np.random.default_rng(n)
        nrm = rng.standard_normal((n, 4)).astype(np.float32)
        nrm[:, 3] = 0
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        ctr = (rng.standard_normal((n, 4)) * 10).astype(np.float32)
        ctr[:, 3] = 1
        batch = api.Batch(ctr, nrm, rng.uniform(0.002, 0.05, n).astype(np.float32), np.full(n, a.ids, np.int32),
                          rng.integers(0, 200, (n, a.ids)).astype(np.int32))
        batch.color[...] = rng.uniform(0, 255.99, (n, 3)).astype(np.float32)
        raw = os.path.join(shm, "patches.raw")
        with open(raw, "wb") as f:
            f.write(np.array([n, a.ids], np.int32).tobytes())
            for x in (batch.center, batch.normal, batch.scale, batch.color, batch.n_images, batch.images):
                f.write(x.tobytes())
        b = batch.c_struct()
        for binary in (False, True):
            flags = api.ply_flags(binary=binary)
            size = C.c_size_t(0)
            api._chk(L.hpmvs_ply_ext_batch(0, C.byref(b), None, 0, flags, None, 0, C.byref(size), 0, None))
            total = size.value
            out = np.empty(total, np.uint8)
            api._chk(L.hpmvs_ply_ext_batch(0, C.byref(b), None, 0, flags, out.ctypes.data, out.nbytes, C.byref(size), 0, None))
            header = out[:1024].tobytes().index(b"end_header\n") + len(b"end_header\n")
            # the vertex section: n fixed records, or the text up to the n-th newline
            vertex_bytes = 31 * n if binary else int(np.flatnonzero(out[header:] == 10)[n - 1]) + 1
            list_bytes = total - header - vertex_bytes
            ms = (C.c_float * 6)()
            stage = {k: [] for k in STAGES}
            wall, timed_wall, api_wall, host = [], [], [], []
            ply = os.path.join(shm, "host.ply")
            for rep in range(a.warmup + a.reps):   # the sides alternate, so that what else runs on the host falls on both
                t = time.perf_counter()
                api._chk(L.hpmvs_ply_ext_timed(0, C.byref(b), None, 0, flags, out.ctypes.data, out.nbytes, C.byref(size), ms))
                t1 = time.perf_counter()
                api._chk(L.hpmvs_ply_ext_batch(0, C.byref(b), None, 0, flags, out.ctypes.data, out.nbytes, C.byref(size), 0, None))
                t2 = time.perf_counter()
                api.ply_ext(batch, binary=binary)   # what a Python caller pays: the size query, then the call
                t3 = time.perf_counter()
                if rep >= a.warmup:
                    for k, v in zip(STAGES, ms):
                        stage[k].append(float(v))
                    timed_wall.append(1e3 * (t1 - t))
                    wall.append(1e3 * (t2 - t1))
                    api_wall.append(1e3 * (t3 - t2))
                if rep < a.host_reps:
                    r = subprocess.run([exe, raw, ply, str(int(binary)), "1"], check=True, capture_output=True, text=True)
                    host.append(float(r.stdout.split()[1]))
            with open(ply, "rb") as f:
                equal = f.read() == out[:size.value].tobytes()
            os.remove(ply)
            # the ceiling: a plain device-to-device copy of the same byte count
            src = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)
            dst.copy_(src)
            torch.cuda.synchronize()
            d2d = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                d2d.append(e0.elapsed_time(e1))
            del src, dst
            r = {"patches": n, "binary": binary, "file_bytes": total, "vertex_bytes": vertex_bytes, "list_bytes": list_bytes,
                 "device_file_equals_host_file": bool(equal), "stages": {k: med(v) for k, v in stage.items()},
                 "device_call_wall_ms": med(wall), "device_timed_call_wall_ms": med(timed_wall),
                 "api_ply_ext_wall_ms": med(api_wall), "host_writeExtPly_ms": med(host),
                 "d2d_copy_same_bytes_ms": med(d2d)}
            r["host_over_device"] = r["host_writeExtPly_ms"]["median"] / r["device_call_wall_ms"]["median"]
            r["host_over_api_ply_ext"] = r["host_writeExtPly_ms"]["median"] / r["api_ply_ext_wall_ms"]["median"]
            r["vertex_kernel_GBps"] = vertex_bytes / (1e6 * max(r["stages"]["vertex_kernel_ms"]["median"], 1e-6))
            r["list_kernel_GBps"] = list_bytes / (1e6 * max(r["stages"]["list_kernel_ms"]["median"], 1e-6))
            r["d2d_copy_GBps"] = total / (1e6 * max(r["d2d_copy_same_bytes_ms"]["median"], 1e-6))
            res["runs"].append(r)
        os.remove(raw)
    os.remove(exe)
    os.rmdir(bin_dir)
    os.rmdir(shm)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
