"""hpmvs_octree_locate_batch at production size: 98 304 points (the six extend candidates of 16 384 leaves before optimize)
against the seed tree of the 50-view 4K scene.  Wall time of the host-pointer call and of the device-pointer call, the outputs of
both compared byte for byte, the tree's size.  Writes profiles/octree_locate_scale.json and prints it as one JSON line; the figure
it stands beside -- what the C++ walk spends on the candidates' leaves for the same count -- is copied from
profiles/walk_unify_extend_level.json, not measured again.

    python tools/octree_locate_scale.py [views w h seeds leaves]        (default: 50 3840 2160 100000 16384)
    python tools/octree_locate_scale.py --calls-only [views w h seeds leaves]   the device-pointer call alone, three times: run
                                                                        THIS under `rocprofv3 --kernel-trace --stats`
    python tools/octree_locate_scale.py --kernel-stats stats.csv        enter that run's kernel times into the record"""
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORD = os.path.join(ROOT, "profiles", "octree_locate_scale.json")
PATCH_INIT_MAXLEVEL = 9
OUTPUTS = (("inside", np.uint8, 1), ("leaf_key", np.uint64, 1), ("leaf_index", np.int32, 1), ("leaf_width", np.float32, 1),
           ("leaf_center", np.float32, 3), ("target_key", np.uint64, 1))


def seed_tree(g, scene, V, NS):
    from hpmvs_amd import api, frontier, synth
    seeds = synth.make_seeds(scene, NS, start_level=4, max_images=min(V, api.MAX_IMAGES))
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(g, b)
    ok = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[ok], b.normal[ok], b.scale[ok], b.n_images[ok], b.images[ok])
    R.ok[:] = 1
    return R, frontier.seed_tree(g, R, PATCH_INIT_MAXLEVEL, set_depths=False)


def path_keys(T):
    """Leaf and branch keys of a SeedTree, all leaves at once: descend to every cell_center for cell_level levels with
    Cell(parent, idx) (double arithmetic, float storage); the branches are the proper prefixes."""
    L = T.n_leaves
    c = np.tile(np.asarray(T.root_center, np.float32), (L, 1))
    w = np.float32(T.root_width)
    key = np.ones(L, np.uint64)
    for d in range(int(T.cell_level.max()) if L else 0):
        live = T.cell_level > d
        bits = T.cell_center > c
        idx = (bits[:, 0].astype(np.uint64) | (bits[:, 1].astype(np.uint64) << np.uint64(1)) | (bits[:, 2].astype(np.uint64) << np.uint64(2)))
        key = np.where(live, (key << np.uint64(3)) | idx, key)
        w = np.float32(float(w) / 2.0)
        step = np.where(bits, 1.0, -1.0) * float(w) / 2.0
        c = np.where(live[:, None], (c.astype(np.float64) + step).astype(np.float32), c)
    branches = set()
    k = key.copy()
    while (k > np.uint64(15)).any():
        k = np.where(k > np.uint64(15), k >> np.uint64(3), k)
        branches.update(np.unique(k[k > np.uint64(7)]).tolist())
    return np.array(sorted(branches), np.uint64), key


def candidates(g, R, T, n_leaves):
    """The six extend candidates before optimize of the first `n_leaves` leaves' first patches, and addConditional's widths."""
    from hpmvs_amd import api, frontier
    n = min(n_leaves, T.n_leaves)
    rows = T.rows[T.cell_start[:n]]
    P = frontier._rows(R, rows)
    pre = api.expand_batch(g, api.EXPAND_EXTEND, P, np.zeros((n, 3), np.float32), T.cell_width[:n], np.ones(6 * n, np.uint8))
    aw = np.repeat((T.cell_width[:n].astype(np.float64) * 0.9).astype(np.float32), 6)
    return np.ascontiguousarray(pre.center[:, :3]), aw


def device_call(g, T, bk, lk, pts, aw):
    import torch
    from hpmvs_amd import api
    dev = "cuda"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev)
    tb, tl, tp, ta = up(bk, np.int64), up(lk, np.int64), up(pts, np.float32), up(aw, np.float32)
    n = len(pts)
    outs = [torch.zeros(n * k * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev) for _, dt, k in OUTPUTS]
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(T.root_center[k])
    t.root_width = float(T.root_width)
    t.n_branches, t.n_leaves = len(bk), len(lk)
    t.branch_key, t.leaf_key = tb.data_ptr(), tl.data_ptr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = api.lib().hpmvs_octree_locate_batch(g.h, C.byref(t), n, tp.data_ptr(), ta.data_ptr(), *[o.data_ptr() for o in outs], 1, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(api.lib().hpmvs_last_error().decode())
    return dt, [o.cpu().numpy().tobytes() for o in outs]


def main(argv):
    if argv and argv[0] == "--kernel-stats":
        with open(RECORD) as f:
            rec = json.load(f)
        rows = {}
        with open(argv[1]) as f:
            for r in csv.DictReader(f):
                if "octree_" in r["Name"]:
                    rows[r["Name"].split("(")[0][:64]] = {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
        rec["kernels_of_3_calls"] = rows
        rec["kernel_us_per_call"] = round(sum(v["total_us"] for v in rows.values()) / 3, 1)
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return rec
    import torch
    from hpmvs_amd import api, synth
    calls_only = bool(argv) and argv[0] == "--calls-only"
    if calls_only:
        argv = argv[1:]
    V, W_, H_, NS, NL = (int(a) for a in argv[:5]) if len(argv) >= 5 else (50, 3840, 2160, 100000, 16384)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    bk, lk = path_keys(T)
    pts, aw = candidates(g, R, T, NL)
    if calls_only:
        for _ in range(3):
            device_call(g, T, bk, lk, pts, aw)
        print(json.dumps({"calls_only": True, "points": len(pts)}))
        return None
    api.octree_locate_batch(g, T.root_center, T.root_width, bk, lk, pts, aw)   # warm-up
    host, dev = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        r = api.octree_locate_batch(g, T.root_center, T.root_width, bk, lk, pts, aw)
        host.append(time.perf_counter() - t0)
        dt, raw = device_call(g, T, bk, lk, pts, aw)
        dev.append(dt)
    same = raw == [getattr(r, name).tobytes() for name, _, _ in OUTPUTS]
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "branches": int(len(bk)), "depth_histogram": {str(d): int(c) for d, c in enumerate(np.bincount(T.cell_level)) if c},
           "points": int(len(pts)), "inside": int(r.inside.sum()), "in_nonempty_leaf": int((r.leaf_index >= 0).sum()),
           "add_conditional_refuses": int((r.target_key == 0).sum()),
           "host_pointer_call_ms_median": round(1e3 * float(np.median(host)), 3),
           "device_pointer_call_ms_median": round(1e3 * float(np.median(dev)), 3),
           "host_and_device_pointer_outputs_equal_bytes": bool(same)}
    prior = os.path.join(ROOT, "profiles", "walk_unify_extend_level.json")
    if os.path.exists(prior):
        with open(prior) as f:
            rec["cpp_walk_candidates_leaves_ms_recorded"] = json.load(f).get("candidates' leaves (ms)")
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
