"""hpmvs_border_forest_batch at production size: 1e4 and 1e5 border patches against the seed tree of the 50-view 4K scene, cut by
hpmvs_octree_partition(min_trees=100).  The patches are made as in tools/octree_insert_scale.py -- refined survivors displaced by up
to two of their own cells in a random direction -- and keep their normals and image lists, so that the accepted ones write depths.

  (a) the per-tree path: ONE hpmvs_octree_route_batch over the roots, then per destination tree ONE hpmvs_octree_insert_batch on
      that tree's keys with its rows and ONE hpmvs_set_depths_batch over the accepted ones -- the device calls of
      frontier.route_border and frontier.insert_border, without the Octree bookkeeping that both paths share
  (b) the one call, with host pointers and with device pointers
  (c) octree.hpp's border_forest_sequential compiled by g++ -O2 on one thread (tests/border_forest_host.cpp; its time includes the
      table build, as the call's does; it writes no depths)

(a) and (b) alternate five times after a warm-up, from freshly reset depth maps (the reset is not timed); medians and min / max.
The outputs of (a), (b) and (c) are compared byte for byte.  Writes profiles/border_forest_scale.json and prints it as one JSON
line.

    python tools/border_forest_scale.py [views w h seeds]               (default: 50 3840 2160 100000)
    python tools/border_forest_scale.py --calls-only [views w h seeds]  the device-pointer call alone, three times each size: run
                                                                        THIS under `rocprofv3 --kernel-trace --stats`
    python tools/border_forest_scale.py --kernel-stats stats.csv        enter that run's kernel times into the record"""
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
RECORD = os.path.join(ROOT, "profiles", "border_forest_scale.json")
SIZES = (10000, 100000)
NAMES = ("tree", "accepted", "leaf_key", "blocker")


def border_batch(rng, R, n):
    """n refined survivors (with replacement) displaced by up to two of their cells, as a patch batch"""
    from hpmvs_amd import api
    rows = rng.integers(0, R.n, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    step = rng.uniform(0.5, 2.0, n) * 2.0 * R.scale[rows].astype(np.float64)
    center = R.center[rows].copy()
    center[:, :3] = (R.center[rows, :3].astype(np.float64) + d * step[:, None]).astype(np.float32)
    return api.Batch(center, R.normal[rows], R.scale[rows], R.n_images[rows], R.images[rows])


def per_tree_path(g, flat, border):
    """(a) -> (seconds, [tree, accepted, leaf_key, blocker] as bytes, destination trees)"""
    from hpmvs_amd import api, frontier
    roots, bf, lf, bk, lk = flat
    n = border.n
    accepted, leaf_key, blocker = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    add_width = (border.scale.astype(np.float64) * 2.0).astype(np.float32)
    t0 = time.perf_counter()
    tree = api.octree_route_batch(g, roots, border.center[:, :3])
    dest = np.unique(tree[tree >= 0])
    for k in dest:
        rows = np.nonzero(tree == k)[0]
        r = api.octree_insert_batch(g, roots[k, :3], roots[k, 3], bk[bf[k]:bf[k + 1]], lk[lf[k]:lf[k + 1]], border.center[rows, :3], add_width[rows])
        acc = rows[r.accepted != 0]
        if len(acc):
            batch = frontier._rows(border, acc)
            batch.ok[:] = 1
            api.set_depths_batch(g, batch)
        accepted[rows], leaf_key[rows] = r.accepted, r.leaf_key
        blocker[rows] = np.where(r.blocker < 0, -1, rows[np.maximum(r.blocker, 0)])
    dt = time.perf_counter() - t0
    return dt, [tree.tobytes(), accepted.tobytes(), leaf_key.tobytes(), blocker.tobytes()], int(len(dest))


def one_call_host(g, flat, border):
    from hpmvs_amd import api
    t0 = time.perf_counter()
    r = api.border_forest_batch(g, border, *flat, set_depths=True)
    return time.perf_counter() - t0, [getattr(r, name).tobytes() for name in NAMES]


class DeviceCall:
    """the one call with device pointers: everything uploaded once, the call alone timed"""

    def __init__(self, g, flat, border):
        import torch
        from hpmvs_amd import api
        self.g, self.torch = g, torch
        roots, bf, lf, bk, lk = flat
        self.host = (np.ascontiguousarray(roots), np.ascontiguousarray(bf), np.ascontiguousarray(lf))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.keep = [up(bk), up(lk)] + [up(getattr(border, name)) for name in ("center", "normal", "scale", "n_images", "images")]
        n = border.n
        self.out = [torch.zeros(n * k, dtype=torch.uint8, device="cuda") for k in (4, 1, 8, 4)]
        self.f = api.OctreeForest()
        self.f.n_trees = len(roots)
        self.f.root, self.f.branch_first, self.f.leaf_first = (a.ctypes.data for a in self.host)
        self.f.branch_key, self.f.leaf_key = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        self.pb = api.PatchBatch()
        self.pb.n, self.pb.max_images = n, border.max_images
        for name, t in zip(("center", "normal", "scale", "n_images", "images"), self.keep[2:]):
            setattr(self.pb, name, t.data_ptr())
        self.res = api.BorderForestResultStruct()
        for name, t in zip(NAMES, self.out):
            setattr(self.res, name, t.data_ptr())
        torch.cuda.synchronize()

    def run(self):
        from hpmvs_amd import api
        t0 = time.perf_counter()
        rc = api.lib().hpmvs_border_forest_batch(self.g.h, C.byref(self.f), C.byref(self.pb), 1, C.byref(self.res), 1, None)
        self.torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(api.lib().hpmvs_last_error().decode())
        return dt, [o.cpu().numpy().tobytes() for o in self.out]


def host_build(build_dir):
    so = os.path.join(build_dir, "libborder_forest_host.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "border_forest_host.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.bf_border.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 7
    return L


def sequential_host(L, flat, border):
    """(c) -> (seconds, outputs as bytes)"""
    roots, bf, lf, bk, lk = (np.ascontiguousarray(a) for a in flat)
    n = border.n
    out = [np.zeros(n, dt) for dt in (np.int32, np.uint8, np.uint64, np.int32)]
    found = np.zeros(2, np.int32)
    t0 = time.perf_counter()
    rc = L.bf_border(len(roots), roots.ctypes.data, bf.ctypes.data, lf.ctypes.data, bk.ctypes.data, lk.ctypes.data, n, border.center.ctypes.data,
                     border.scale.ctypes.data, *[a.ctypes.data for a in out], found.ctypes.data)
    dt = time.perf_counter() - t0
    assert rc == 0, found
    return dt, [a.tobytes() for a in out]


def _ms(times):
    return {"median": round(1e3 * float(np.median(times)), 3), "min": round(1e3 * float(min(times)), 3), "max": round(1e3 * float(max(times)), 3)}


def main(argv):
    if argv and argv[0] == "--kernel-stats":
        with open(RECORD) as f:
            rec = json.load(f)
        rows = {}
        with open(argv[1]) as f:
            for r in csv.DictReader(f):
                name = "rocprim (the radix sorts)" if "rocprim" in r["Name"] else r["Name"].split("(")[0] if any(
                    k in r["Name"] for k in ("border_forest_", "forest_build", "forest_check", "set_depths_kernel")) else None
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
    from hpmvs_amd import api, frontier, synth
    from octree_locate_scale import seed_tree
    calls_only = bool(argv) and argv[0] == "--calls-only"
    if calls_only:
        argv = argv[1:]
    V, W_, H_, NS = (int(a) for a in argv[:4]) if len(argv) >= 4 else (50, 3840, 2160, 100000)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    P = frontier.partition(g, frontier.Octree.from_seed_tree(T), min_trees=100)
    flat = frontier._flatten_forest(P.trees)
    rng = np.random.default_rng(1)
    api.depth_reset(g)
    if calls_only:
        for n in SIZES:
            call = DeviceCall(g, flat, border_batch(rng, R, n))
            for _ in range(3):
                call.run()
        print(json.dumps({"calls_only": True, "sizes": SIZES}))
        return None
    L = host_build(tempfile.mkdtemp())
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "subtrees": len(P.trees), "forest_branch_keys": int(len(flat[3])), "forest_leaf_keys": int(len(flat[4])), "sizes": {}}
    for n in SIZES:
        border = border_batch(rng, R, n)
        call = DeviceCall(g, flat, border)
        per_tree_path(g, flat, border); one_call_host(g, flat, border); call.run()   # warm-up
        a, bh, bd = [], [], []
        for _ in range(5):
            api.depth_reset(g)
            ta, out_a, dest = per_tree_path(g, flat, border)
            api.depth_reset(g)
            th, out_h = one_call_host(g, flat, border)
            api.depth_reset(g)
            td, out_d = call.run()
            a.append(ta); bh.append(th); bd.append(td)
        seq = [sequential_host(L, flat, border) for _ in range(3)]
        tree = np.frombuffer(out_h[0], np.int32)
        acc = np.frombuffer(out_h[1], np.uint8)
        blk = np.frombuffer(out_h[3], np.int32)
        spread = max(a) - min(a)
        s = {"destination_trees": dest, "unrouted": int((tree < 0).sum()), "accepted": int(acc.sum()),
             "refused_by_the_tree": int(((acc == 0) & (blk < 0) & (tree >= 0)).sum()), "refused_by_an_earlier_patch": int((blk >= 0).sum()),
             "a_route_plus_insert_per_tree_ms": _ms(a), "b_one_call_host_pointers_ms": _ms(bh), "b_one_call_device_pointers_ms": _ms(bd),
             "c_border_forest_sequential_gxx_1_thread_ms": _ms([t for t, _ in seq]),
             "b_host_within_a_median_plus_a_spread": bool(np.median(bh) <= np.median(a) + spread),
             "b_device_within_a_median_plus_a_spread": bool(np.median(bd) <= np.median(a) + spread),
             "a_equals_b_host_bytes": bool(out_a == out_h), "b_host_equals_b_device_bytes": bool(out_h == out_d),
             "b_equals_c_bytes": bool(out_h == seq[0][1])}
        rec["sizes"][str(n)] = s
        print(json.dumps({str(n): s}), flush=True)
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
