"""hpmvs_octree_insert_batch and hpmvs_octree_route_batch at production size: 1e4 and 1e5 border patches against the seed tree
of the 50-view 4K scene.  The patches are refined survivors displaced by up to two of their own cells in a random direction --
points just outside and just inside the cells next to them, as a neighbouring subtree's border candidates arrive -- with
addConditional's width scale_3dx_ * 2.0 from their refined scales; the routing runs over the 64 cells of depth 2 as subtree roots.
Wall time of the host-pointer and of the device-pointer call, both outputs compared byte for byte, beside the two sequential
loops on the same patches: (a) a Python loop of frontier.Octree.add_conditional, (b) octree.hpp's insert_sequential compiled by
g++ -O2 on one thread (tests/octree_insert_host.cpp; its time includes the table build, as the call's does).  Writes
profiles/octree_insert_scale.json and prints it as one JSON line.

    python tools/octree_insert_scale.py [views w h seeds]               (default: 50 3840 2160 100000)
    python tools/octree_insert_scale.py --calls-only [views w h seeds]  the device-pointer calls alone, three times each size: run
                                                                        THIS under `rocprofv3 --kernel-trace --stats`
    python tools/octree_insert_scale.py --kernel-stats stats.csv        enter that run's kernel times into the record"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
RECORD = os.path.join(ROOT, "profiles", "octree_insert_scale.json")
SIZES = (10000, 100000)
PYTHON_LOOP_MAX = 100000   # (a) is run up to this many patches


def border_patches(rng, R, n):
    """n refined survivors (with replacement) displaced by up to two of their cells; add_width = (float)(scale * 2.0)"""
    rows = rng.integers(0, R.n, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    step = rng.uniform(0.5, 2.0, n) * 2.0 * R.scale[rows].astype(np.float64)
    pts = (R.center[rows, :3].astype(np.float64) + d * step[:, None]).astype(np.float32)
    return np.ascontiguousarray(pts), (R.scale[rows].astype(np.float64) * 2.0).astype(np.float32)


def depth2_roots(center, width):
    """the 64 cells of depth 2 as [64][4] roots (c_, width_), Cell(parent, idx) arithmetic"""
    from hpmvs_amd.frontier import child_cell
    out = []
    for i in range(8):
        c1, w1 = child_cell(np.asarray(center, np.float32), np.float32(width), i)
        for j in range(8):
            c2, w2 = child_cell(c1, w1, j)
            out.append([*c2, w2])
    return np.array(out, np.float32)


def device_calls(g, T, bk, lk, pts, aw, roots):
    """the two calls with device pointers -> (insert seconds, route seconds, outputs as bytes)"""
    import torch
    from hpmvs_amd import api
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to("cuda")
    tb, tl, tp, ta = up(bk, np.int64), up(lk, np.int64), up(pts, np.float32), up(aw, np.float32)
    n = len(pts)
    acc, key, blk, to = (torch.zeros(n * k, dtype=torch.uint8, device="cuda") for k in (1, 8, 4, 4))
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(T.root_center[k])
    t.root_width = float(T.root_width)
    t.n_branches, t.n_leaves = len(bk), len(lk)
    t.branch_key, t.leaf_key = tb.data_ptr(), tl.data_ptr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = api.lib().hpmvs_octree_insert_batch(g.h, C.byref(t), n, tp.data_ptr(), ta.data_ptr(), acc.data_ptr(), key.data_ptr(), blk.data_ptr(), 1, None)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rc = rc or api.lib().hpmvs_octree_route_batch(g.h, len(roots), roots.ctypes.data, n, tp.data_ptr(), to.data_ptr(), 1, None)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if rc != 0:
        raise RuntimeError(api.lib().hpmvs_last_error().decode())
    return t1 - t0, t2 - t1, [o.cpu().numpy().tobytes() for o in (acc, key, blk, to)]


def host_build(build_dir):
    so = os.path.join(build_dir, "liboctree_insert_host.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "octree_insert_host.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.ot_insert.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return L


def sequential_host(L, T, bk, lk, pts, aw):
    """(b): -> (seconds, outputs as bytes)"""
    n = len(pts)
    root = np.array([*T.root_center, T.root_width], np.float32)
    acc, key, blk = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    t0 = time.perf_counter()
    rc = L.ot_insert(root.ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, n, pts.ctypes.data, aw.ctypes.data,
                     acc.ctypes.data, key.ctypes.data, blk.ctypes.data)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, [acc.tobytes(), key.tobytes(), blk.tobytes()]


def python_loop(T, bk, lk, pts, aw):
    """(a): -> (seconds, accepted as bytes)"""
    from hpmvs_amd import frontier
    tree = frontier.Octree(T.root_center, T.root_width)
    tree.branches = set(bk.tolist())
    for j, k in enumerate(lk.tolist()):
        tree.leaves[k] = j
        tree._count(k, +1)
    acc = np.zeros(len(pts), np.uint8)
    t0 = time.perf_counter()
    for i in range(len(pts)):
        acc[i] = tree.add_conditional(pts[i], aw[i], ("border", i)) is not None
    return time.perf_counter() - t0, acc.tobytes()


def main(argv):
    if argv and argv[0] == "--kernel-stats":
        with open(RECORD) as f:
            rec = json.load(f)
        rows = {}
        with open(argv[1]) as f:
            for r in csv.DictReader(f):
                name = "rocprim (the radix sort)" if "rocprim" in r["Name"] else r["Name"].split("(")[0] if "octree_" in r["Name"] else None
                if name:
                    e = rows.setdefault(name, {"calls": 0, "total_us": 0.0})
                    e["calls"] += int(r["Calls"])
                    e["total_us"] = round(e["total_us"] + float(r["TotalDurationNs"]) / 1e3, 1)
        rec["kernels_of_3_calls_of_each_size"] = rows
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return rec
    import torch
    from hpmvs_amd import api, synth
    from octree_locate_scale import path_keys, seed_tree
    calls_only = bool(argv) and argv[0] == "--calls-only"
    if calls_only:
        argv = argv[1:]
    V, W_, H_, NS = (int(a) for a in argv[:4]) if len(argv) >= 4 else (50, 3840, 2160, 100000)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    bk, lk = path_keys(T)
    lk = np.ascontiguousarray(lk)
    roots = depth2_roots(T.root_center, T.root_width)
    rng = np.random.default_rng(1)
    if calls_only:
        for n in SIZES:
            pts, aw = border_patches(rng, R, n)
            for _ in range(3):
                device_calls(g, T, bk, lk, pts, aw, roots)
        print(json.dumps({"calls_only": True, "sizes": SIZES}))
        return None
    L = host_build(tempfile.mkdtemp())
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "branches": int(len(bk)), "subtree_roots": int(len(roots)), "sizes": {}}
    for n in SIZES:
        pts, aw = border_patches(rng, R, n)
        api.octree_insert_batch(g, T.root_center, T.root_width, bk, lk, pts, aw)   # warm-up
        host, dev, route_host, route_dev = [], [], [], []
        for _ in range(5):
            t0 = time.perf_counter()
            r = api.octree_insert_batch(g, T.root_center, T.root_width, bk, lk, pts, aw)
            t1 = time.perf_counter()
            to = api.octree_route_batch(g, roots, pts)
            route_host.append(time.perf_counter() - t1)
            host.append(t1 - t0)
            di, dr, raw = device_calls(g, T, bk, lk, pts, aw, roots)
            dev.append(di); route_dev.append(dr)
        ours = [r.accepted.tobytes(), r.leaf_key.tobytes(), r.blocker.tobytes()]
        seq = [sequential_host(L, T, bk, lk, pts, aw) for _ in range(3)]
        members = (r.accepted != 0) | (r.blocker >= 0)
        static_leaf = np.unique(api.octree_locate_batch(g, T.root_center, T.root_width, bk, lk, pts[members]).leaf_key, return_counts=True)[1]
        s = {"accepted": int(r.accepted.sum()), "refused_by_the_tree": int(((r.accepted == 0) & (r.blocker < 0)).sum()),
             "refused_by_an_earlier_patch": int((r.blocker >= 0).sum()), "routed": int((to >= 0).sum()),
             "runs": int(len(static_leaf)), "longest_run": int(static_leaf.max()) if len(static_leaf) else 0,
             "host_pointer_call_ms_median": round(1e3 * float(np.median(host)), 3),
             "device_pointer_call_ms_median": round(1e3 * float(np.median(dev)), 3),
             "route_host_pointer_call_ms_median": round(1e3 * float(np.median(route_host)), 3),
             "route_device_pointer_call_ms_median": round(1e3 * float(np.median(route_dev)), 3),
             "insert_sequential_gxx_1_thread_ms_median": round(1e3 * float(np.median([t for t, _ in seq])), 3),
             "host_and_device_pointer_outputs_equal_bytes": bool(raw == ours + [to.tobytes()]),
             "equals_insert_sequential_bytes": bool(seq[0][1] == ours)}
        if n <= PYTHON_LOOP_MAX:
            dt, acc = python_loop(T, bk, lk, pts, aw)
            s["python_add_conditional_loop_ms"] = round(1e3 * dt, 1)
            s["equals_python_loop_decisions"] = bool(acc == ours[0])
        rec["sizes"][str(n)] = s
        print(json.dumps({str(n): s}), flush=True)
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
