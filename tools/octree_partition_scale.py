"""hpmvs_octree_partition at production size: the seed tree of the bench's default scene (50 views 4K) with 1e6 seed points
through init_patches_batch and seed_tree, split with min_trees = 100 (the reference's --subtrees) and min_split_leaves = 100.
Wall time of the device-pointer and of the host-pointer call, best of four each, beside octree.hpp's host restatement compiled by
g++ -O2 on one thread on the same keys (tests/octree_partition_host.cpp; its time includes the table build and the sort, as the
call's does); all outputs compared byte for byte.  Writes profiles/octree_partition_scale.json and prints it as one JSON line.

    python tools/octree_partition_scale.py [views w h seeds]      (default: 50 3840 2160 1000000)"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
RECORD = os.path.join(ROOT, "profiles", "octree_partition_scale.json")
MIN_TREES, MIN_SPLIT_LEAVES, RUNS = 100, 100, 4


def device_call(g, T, bk, lk, opr):
    """the call with device pointers -> (seconds, Arrays)"""
    import torch
    from hpmvs_amd import api
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    r = opr.Arrays(len(bk), len(lk), MIN_TREES)
    tb, tl = up(bk), up(lk)
    outs = [up(getattr(r, name)) for name, _, _ in opr.OUTPUTS]
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(T.root_center[k])
    t.root_width = float(T.root_width)
    t.n_branches, t.n_leaves = len(bk), len(lk)
    t.branch_key, t.leaf_key = tb.data_ptr(), tl.data_ptr()
    info = api.OctreePartitionInfo()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = api.lib().hpmvs_octree_partition(g.h, C.byref(t), MIN_TREES, MIN_SPLIT_LEAVES, C.byref(info), *[o.data_ptr() for o in outs], 1, None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(api.lib().hpmvs_last_error().decode())
    for (name, dtype, _), o in zip(opr.OUTPUTS, outs):
        a = getattr(r, name)
        a[...] = o.cpu().numpy().view(dtype).reshape(a.shape)
    r.info[:] = np.frombuffer(bytes(info), np.int32)
    return dt, r


def main(argv):
    import torch
    import octree_partition_ref as opr
    from hpmvs_amd import api, frontier, synth
    from octree_locate_scale import PATCH_INIT_MAXLEVEL, path_keys
    V, W_, H_, NS = (int(a) for a in argv[:4]) if len(argv) >= 4 else (50, 3840, 2160, 1000000)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    xyz, off, img = synth.make_nvm_points(scene, NS, start_level=4)
    batch = api.init_patches_batch(g, xyz, off, img, start_level=4, max_images=min(V, api.FAST_IMAGES))
    T = frontier.seed_tree(g, batch, PATCH_INIT_MAXLEVEL, set_depths=False)
    bk, lk = path_keys(T)
    bk, lk = np.ascontiguousarray(bk), np.ascontiguousarray(lk)
    host = opr.HostPartition(tempfile.mkdtemp())
    seq = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        rc, want = host.partition(T.root_center, T.root_width, bk, lk, MIN_TREES, MIN_SPLIT_LEAVES)
        seq.append(time.perf_counter() - t0)
        assert rc == 0
    try:
        api.octree_partition(g, T.root_center, T.root_width, bk, lk, MIN_TREES, MIN_SPLIT_LEAVES)   # warm-up
    except api.HpmvsError as e:   # (a table that outgrows the scene's launch workspace is refused: record that instead of times)
        rec = {"scene": f"{V} x {W_}x{H_}", "seed_points": NS, "leaves": int(len(lk)), "branches": int(len(bk)), "refused": str(e),
               "partition_sequential_gxx_O2_1_thread_ms_best_of_4": round(1e3 * min(seq), 3)}
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return rec
    dev, hst = [], []
    for _ in range(RUNS):
        dt, got = device_call(g, T, bk, lk, opr)
        dev.append(dt)
        t0 = time.perf_counter()
        P = api.octree_partition(g, T.root_center, T.root_width, bk, lk, MIN_TREES, MIN_SPLIT_LEAVES)
        hst.append(time.perf_counter() - t0)
    n = int(want.info[0])
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seed_points": NS, "survivors": int(batch.ok.astype(bool).sum()),
           "leaves": int(len(lk)), "branches": int(len(bk)), "min_trees": MIN_TREES, "min_split_leaves": MIN_SPLIT_LEAVES,
           "n_trees": n, "n_orphans": int(want.info[1]), "n_splits": int(want.info[2]), "stop": int(want.info[3]),
           "histogram": want.info[4:].tolist(), "largest_subtrees": sorted(want.tree_leaves[:n].tolist(), reverse=True)[:5],
           "device_pointer_call_ms_best_of_4": round(1e3 * min(dev), 3), "host_pointer_call_ms_best_of_4": round(1e3 * min(hst), 3),
           "partition_sequential_gxx_O2_1_thread_ms_best_of_4": round(1e3 * min(seq), 3),
           "device_pointer_outputs_equal_the_host_restatement_bytes": not got.differences(want),
           "host_pointer_outputs_equal_the_host_restatement_bytes": bool(
               all(getattr(P, name).tobytes() == getattr(want, name).tobytes() for name, _, _ in opr.OUTPUTS)
               and [P.n_trees, P.n_orphans, P.n_splits, P.stop] + P.histogram.tolist() == want.info.tolist())}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
