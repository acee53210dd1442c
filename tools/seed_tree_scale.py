"""The seed octree (hpmvs_seed_tree_batch, the second half of Scene::initPatches, reference Scene.cpp:183-199) at production size:
the survivors of the seed loop on the 50-view 4K scene, 1e5 and 1e6 seeds.  Per size: wall time of the host-pointer call and of the
device-pointer call (tree only, set_depths = 0), the single-thread pointer-octree loop of tools/seed_tree_host.cpp (add + flatten, as
the reference runs it), the tables of both compared byte for byte, leaf count and depth histogram.  Writes
profiles/seed_tree_scale.json and prints it as one JSON line.

    python tools/seed_tree_scale.py [views w h [seeds ...]]            (default: 50 3840 2160 100000 1000000)
    python tools/seed_tree_scale.py --calls-only views w h seeds       the calls alone, three times: run THIS under
                                                                       `rocprofv3 --kernel-trace --stats` (a run of its own)
    python tools/seed_tree_scale.py --kernel-stats seeds stats.csv     enter that run's kernel times into the record

The Python restatement's time for 1e5 seeds is the one profiles/filter_level_scale.json already records
(tree_s_python_restatement); it is copied, not measured again."""
import csv
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
RECORD = os.path.join(ROOT, "profiles", "seed_tree_scale.json")
PATCH_INIT_MAXLEVEL = 9
KERNELS = ("seed_tree_", "rocprim")   # this call's kernels in a trace: its own and rocPRIM's sort / scan


def survivors(g, scene, V, NS):
    from hpmvs_amd import api, synth
    seeds = synth.make_seeds(scene, NS, start_level=4, max_images=min(V, api.MAX_IMAGES))
    b0 = api.Batch.from_seeds(seeds)
    api.optimize_batch(g, b0)
    ok = np.nonzero(b0.ok)[0]
    R = api.Batch(b0.center[ok], b0.normal[ok], b0.scale[ok], b0.n_images[ok], np.full((len(ok), 1), -1, np.int32))
    R.ok[:] = 1
    return R


def device_call(g, R, scale0, outs=None):
    """One device-pointer call on fresh device copies; returns (wall seconds, info, output tensors)."""
    import torch
    from hpmvs_amd import api
    n = R.n
    dev = "cuda"
    tc, ts = torch.from_numpy(R.center).to(dev), torch.from_numpy(scale0.copy()).to(dev)
    o = [torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev),
         torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
         torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev)]
    pb = api.PatchBatch()
    pb.n, pb.max_images = n, 1
    pb.center, pb.scale = tc.data_ptr(), ts.data_ptr()
    info = api.SeedTreeInfo()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = api.lib().hpmvs_seed_tree_batch(g.h, C.byref(pb), PATCH_INIT_MAXLEVEL, 0, C.byref(info), *[t.data_ptr() for t in o], 1, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(api.lib().hpmvs_last_error().decode())
    return dt, info, o, ts


def measure(g, scene, V, NS):
    from hpmvs_amd import api
    R = survivors(g, scene, V, NS)
    n = R.n
    scale0 = R.scale.copy()
    api.seed_tree_batch(g, R, PATCH_INIT_MAXLEVEL, set_depths=False)   # warm-up
    host_walls, dev_walls = [], []
    for _ in range(5):
        R.scale[:] = scale0
        t0 = time.perf_counter()
        info, rows, cs, cc, cw, cl, pc = api.seed_tree_batch(g, R, PATCH_INIT_MAXLEVEL, set_depths=False)
        host_walls.append(time.perf_counter() - t0)
        dev_walls.append(device_call(g, R, scale0)[0])
    L = int(info.n_leaves)
    # the reference's loop: one thread, pointer octree, add + flatten
    so = os.path.join(tempfile.mkdtemp(), "libseed_tree_host.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "seed_tree_host.cpp"),
                    "-o", so], check=True)
    H = C.CDLL(so)
    H.seed_tree_host.restype = C.c_double
    H.seed_tree_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    hroot, hcnt = np.zeros(5, np.float32), np.zeros(2, np.int32)
    hrows, hcs, hcc, hcw, hcl = np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    loops = []
    for _ in range(3):
        hs = scale0.copy()
        loops.append(H.seed_tree_host(n, R.center.ctypes.data, hs.ctypes.data, PATCH_INIT_MAXLEVEL, hroot.ctypes.data, hcnt.ctypes.data,
                                      hrows.ctypes.data, hcs.ctypes.data, hcc.ctypes.data, hcw.ctypes.data, hcl.ctypes.data))
    equal = (int(hcnt[0]) == int(info.n_rows) and int(hcnt[1]) == L and hs.tobytes() == R.scale.tobytes()
             and hrows.tobytes() == rows.tobytes() and hcs[:L + 1].tobytes() == cs[:L + 1].tobytes()
             and hcc[:L].tobytes() == cc[:L].tobytes() and hcw[:L].tobytes() == cw[:L].tobytes() and hcl[:L].tobytes() == cl[:L].tobytes()
             and hroot.tobytes() == np.array(list(info.root_center) + [info.root_width, info.scale_floor], np.float32).tobytes())
    sizes = np.diff(cs[:L + 1])
    return {"seeds": NS, "survivors": n, "leaves": L, "largest_leaf": int(sizes.max()) if L else 0,
            "multi_patch_leaves": int((sizes > 1).sum()), "depth_histogram": {str(d): int(c) for d, c in enumerate(np.bincount(cl[:L])) if c},
            "host_pointer_call_ms_median": round(1e3 * float(np.median(host_walls)), 3),
            "device_pointer_call_ms_median": round(1e3 * float(np.median(dev_walls)), 3),
            "host_loop_1_thread_add_flatten_ms_median": round(1e3 * float(np.median(loops)), 3),
            "tables_equal_host_loop_bytes": bool(equal)}


def load():
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            return json.load(f)
    return {}


def main(argv):
    if argv and argv[0] == "--kernel-stats":
        rec = load()
        rows = {}
        with open(argv[2]) as f:
            for r in csv.DictReader(f):
                if any(k in r["Name"] for k in KERNELS):
                    rows[r["Name"][:96]] = {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
        calls = 3
        for s in rec.get("sizes", []):
            if s["seeds"] == int(argv[1]):
                s["kernels_of_3_calls"] = rows
                s["kernel_us_per_call"] = round(sum(v["total_us"] for v in rows.values()) / calls, 1)
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return rec
    import torch
    from hpmvs_amd import api, synth
    calls_only = bool(argv) and argv[0] == "--calls-only"
    if calls_only:
        argv = argv[1:]
    V, W_, H_ = (int(a) for a in argv[:3]) if len(argv) >= 3 else (50, 3840, 2160)
    sizes = [int(a) for a in argv[3:]] or [100000, 1000000]
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    if calls_only:
        R = survivors(g, scene, V, sizes[0])
        scale0 = R.scale.copy()
        for _ in range(3):
            device_call(g, R, scale0)
        print(json.dumps({"calls_only": True, "seeds": sizes[0], "survivors": R.n}))
        return None
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "PATCH_INIT_MAXLEVEL": PATCH_INIT_MAXLEVEL,
           "sizes": [measure(g, scene, V, NS) for NS in sizes]}
    prior = os.path.join(ROOT, "profiles", "filter_level_scale.json")
    if os.path.exists(prior):
        with open(prior) as f:
            p = json.load(f)
        rec["python_restatement_s_recorded_for"] = {"seeds": p.get("seeds"), "survivors": p.get("survivors"),
                                                    "tree_s_python_restatement": p.get("tree_s_python_restatement")}
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
