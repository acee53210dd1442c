"""One regularize / settle sweep over the subtrees of main's getSubTrees at production size: the 50-view 4K scene and seed set
of tools/extend_level_tree_scale.py, the seed tree cut by hpmvs_octree_partition(min_trees=100), the leaves of the most populated
level (up to 16 384) as cells grouped by subtree, flatness mixed (half regularized, 8 % removed, the rest branched).  Writes
profiles/process_forest_scale.json and prints it as one JSON line.

  (a) the loop a scheduler that follows main makes today: frontier.process_level per subtree that has cells (level_support,
      expand, depth_ops and regularize calls, the versioned table built in Python);
  (b) ONE hpmvs_process_forest_batch over all of them, with host pointers and with device pointers.
After one warm-up of each, (a) and (b) alternate REPS times, wall clock around calls that end synchronised; medians and the spread
(min, max) of each.  The decisions of the two are compared once (flatness bits, removed, split, children: none of them reads the
depth maps, so the runs need not start from the same maps; the maps' equality is the tests' business).  (a) is the baseline: the
same code the parent commit has.
  (c) the C++ host layer, which carries no interpreter cost: the per-tree loop of PatchOptimizer::processLevel beside ONE
      processLevelForest on the same cells (tests/native/bench_process_level_forest.cpp, built here), second pass of each.

    python tools/process_forest_scale.py [views w h seeds leaves min_trees]        (default: 50 3840 2160 100000 16384 100)"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from octree_locate_scale import path_keys, seed_tree  # noqa: E402

RECORD = os.path.join(ROOT, "profiles", "process_forest_scale.json")
REPS = 5
RESULTS = (("support", np.int32, 1), ("removed", np.uint8, 1), ("split", np.uint8, 1), ("children", np.uint8, 4),
           ("child_key", np.uint64, 4), ("n_neighbours", np.int32, 1))


def spread(ts):
    ms = [1e3 * t for t in ts]
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


class Forest:
    """The subtrees as the call takes them, the cells grouped by subtree, and every subtree's snapshot for the loop."""

    def __init__(self, R, T, part, leaves, flatness, final):
        from hpmvs_amd import frontier
        n = part.n_trees
        self.n_trees = n
        self.roots = np.ascontiguousarray(part.root_cell[:n], np.float32)
        border, lorder = np.argsort(part.branch_tree, kind="stable"), np.argsort(part.leaf_tree, kind="stable")
        border, lorder = border[part.branch_tree[border] >= 0], lorder[part.leaf_tree[lorder] >= 0]
        self.branch_key, self.leaf_key = part.branch_sub_key[border].copy(), part.leaf_sub_key[lorder].copy()
        self.branch_first = np.searchsorted(part.branch_tree[border], np.arange(n + 1)).astype(np.int32)
        self.leaf_first = np.searchsorted(part.leaf_tree[lorder], np.arange(n + 1)).astype(np.int32)
        self.patch_center = np.ascontiguousarray(T.patch_center[lorder], np.float32)
        self.cells = frontier._rows(R, T.rows[T.cell_start[leaves]])
        self.cell_tree = np.ascontiguousarray(part.leaf_tree[leaves], np.int32)
        self.cell_key = np.ascontiguousarray(part.leaf_sub_key[leaves], np.uint64)
        self.flatness, self.final = flatness, final
        self.first = np.searchsorted(self.cell_tree, np.arange(n + 1)).astype(np.int64)
        self.with_cells = [k for k in range(n) if self.first[k + 1] > self.first[k]]
        where = np.full(T.n_leaves, -1, np.int64)
        self.per_tree = {}
        self.leaves_of = [lorder[self.leaf_first[k]:self.leaf_first[k + 1]] for k in range(n)]
        self.cell_leaf = np.zeros(len(leaves), np.int32)                 # the cell's leaf among its tree's
        for k in self.with_cells:
            mine = self.leaves_of[k]
            where[mine] = np.arange(len(mine))
            rows = np.arange(self.first[k], self.first[k + 1])
            snap = frontier.OctreeSnapshot(self.roots[k, :3], float(self.roots[k, 3]), T.cell_center[mine], T.cell_width[mine], T.patch_center[mine])
            self.per_tree[k] = (frontier._rows(self.cells, rows), where[leaves[rows]].copy(), snap, rows)
            self.cell_leaf[rows] = where[leaves[rows]]


def loop_host(g, F):
    """(a) -> flatness, removed, split, children over the concatenated queue"""
    from hpmvs_amd import frontier
    n = F.cells.n
    fl, removed, split, children = F.flatness.copy(), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8)
    for k in F.with_cells:
        cells, leaf, snap, rows = F.per_tree[k]
        r = frontier.process_level(g, cells, leaf, F.flatness[rows], np.ones(len(rows), np.uint8), snap, F.final[rows])
        fl[rows] = r.flatness
        st = rows[r.settled]
        removed[st], split[st], children[st] = r.settle.removed, r.settle.split, r.settle.children
    return fl, removed, split, children


def forest_host(g, F):
    from hpmvs_amd import api
    r = api.process_forest_batch(g, F.cells, F.cell_tree, F.cell_key, F.flatness, F.final, F.roots, F.branch_first, F.leaf_first,
                                 F.branch_key, F.leaf_key, F.patch_center)
    return r.flatness, r.removed, r.split, r.children


class DeviceForm:
    """The one call's inputs and outputs on the device."""

    def __init__(self, g, F):
        import torch
        from hpmvs_amd import api
        self.torch, self.api, self.g, self.F = torch, api, g, F
        P, n = F.cells, F.cells.n
        N = 4 * n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.keep = {k: up(getattr(P, k)) for k in api.Batch.FIELDS}
        blank = api.Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                          np.zeros((N, P.max_images), np.int32))
        self.out = {k: up(getattr(blank, k)) for k in api.Batch.FIELDS}
        self.res = {k: torch.zeros(n * w * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for k, dt, w in RESULTS}
        self.ins = {k: up(a) for k, a in dict(bk=F.branch_key, lk=F.leaf_key, pc=F.patch_center, ct=F.cell_tree, ck=F.cell_key, final=F.final).items()}
        self.fl0 = up(F.flatness)
        self.fl = self.fl0.clone()
        self.o = api.default_options()
        self.f = api.OctreeForest()
        self.f.n_trees = F.n_trees
        self.f.root, self.f.branch_first, self.f.leaf_first = F.roots.ctypes.data, F.branch_first.ctypes.data, F.leaf_first.ctypes.data
        self.f.branch_key, self.f.leaf_key = self.ins["bk"].data_ptr(), self.ins["lk"].data_ptr()
        self.pb, self.ob = api.PatchBatch(), api.PatchBatch()
        self.pb.n, self.pb.max_images, self.ob.n, self.ob.max_images = n, P.max_images, N, P.max_images
        for k in api.Batch.FIELDS:
            setattr(self.pb, k, self.keep[k].data_ptr())
            setattr(self.ob, k, self.out[k].data_ptr())
        self.rb = api.ProcessForestResultStruct()
        for k, _, _ in RESULTS:
            setattr(self.rb, k, self.res[k].data_ptr())
        torch.cuda.synchronize()

    def forest(self):
        self.fl.copy_(self.fl0)                                          # flatness is in / out
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = self.api.lib().hpmvs_process_forest_batch(self.g.h, C.byref(self.o), C.byref(self.f), self.ins["pc"].data_ptr(), C.byref(self.pb),
                                                       self.ins["ct"].data_ptr(), self.ins["ck"].data_ptr(), self.fl.data_ptr(),
                                                       self.ins["final"].data_ptr(), C.byref(self.ob), C.byref(self.rb), 1, None)
        if rc != 0:
            raise RuntimeError(self.api.lib().hpmvs_last_error().decode())
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0

    def decisions(self):
        get = lambda t, dt: t.cpu().numpy().view(dt)
        return get(self.fl, np.float32), get(self.res["removed"], np.uint8), get(self.res["split"], np.uint8), get(self.res["children"], np.uint8).reshape(-1, 4)


def cpp_levels(scene, F, T):
    """(c): tests/native/bench_process_level_forest on the same cells -> its JSON line."""
    exe = os.path.join(ROOT, "tests", "native", "bench_process_level_forest")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, exe + ".cpp", "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd",
                    "-Wl,-rpath," + lib], check=True)
    P = F.cells
    dump = os.path.join(os.environ.get("TMPDIR", "/tmp"), "process_forest_scene.bin")
    with open(dump, "wb") as f:
        f.write(struct.pack("i", scene.n_views))
        for v in scene.views:
            f.write(struct.pack("iid4d3d", v.width, v.height, v.f, *v.q, *v.c))
            rgb = v.rgb.cpu().numpy() if hasattr(v.rgb, "cpu") else v.rgb
            f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())
        for lst in scene.covis:
            f.write(struct.pack("i", len(lst)) + struct.pack(f"{len(lst)}i", *lst))
        f.write(struct.pack("i", P.n))
        for k in range(P.n):
            m = int(P.n_images[k])
            f.write(P.center[k].astype(np.float32).tobytes() + P.normal[k].astype(np.float32).tobytes())
            f.write(struct.pack("fi", float(P.scale[k]), m) + struct.pack(f"{m}i", *P.images[k, :m]))
        for i in range(P.n):
            f.write(struct.pack("<fiQBi", float(F.flatness[i]), int(F.cell_tree[i]), int(F.cell_key[i]), int(F.final[i]), int(F.cell_leaf[i])))
        f.write(struct.pack("i", F.n_trees))
        for k in range(F.n_trees):
            bk = F.branch_key[F.branch_first[k]:F.branch_first[k + 1]]
            lk = F.leaf_key[F.leaf_first[k]:F.leaf_first[k + 1]]
            mine = F.leaves_of[k]
            f.write(F.roots[k].tobytes() + struct.pack("i", len(bk)) + bk.tobytes() + struct.pack("i", len(lk)) + lk.tobytes())
            f.write(np.ascontiguousarray(T.cell_center[mine], np.float32).tobytes() + np.ascontiguousarray(T.cell_width[mine], np.float32).tobytes() +
                    np.ascontiguousarray(T.patch_center[mine], np.float32).tobytes())
    try:
        r = subprocess.run([exe, dump], capture_output=True, text=True)
    finally:
        os.remove(dump)
    if r.returncode != 0:
        raise SystemExit(f"bench_process_level_forest failed: {r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def same(a, b):
    return all(np.asarray(x).astype(y.dtype).tobytes() == y.tobytes() for x, y in zip(a, b))


def main(argv):
    import torch
    from hpmvs_amd import api, synth
    V, W_, H_, NS, NL, MT = (int(a) for a in argv[:6]) if len(argv) >= 6 else (50, 3840, 2160, 100000, 16384, 100)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    if T.n_leaves == 0:
        raise SystemExit(f"no seed survived on {V} x {W_}x{H_}: take a larger scene")
    bk, lk = path_keys(T)
    part = api.octree_partition(g, T.root_center, T.root_width, bk, lk, min_trees=MT)
    level = int(np.bincount(T.cell_level).argmax())
    leaves = np.nonzero((T.cell_level == level) & (part.leaf_tree >= 0))[0][:NL]
    leaves = leaves[np.argsort(part.leaf_tree[leaves], kind="stable")]     # the trees' queues one after the other
    rng = np.random.default_rng(7)
    n = len(leaves)
    fl = np.where(rng.random(n) < 0.5, -1.0, 0.0).astype(np.float32)
    rem = rng.random(n) < 0.08
    fl[rem] = np.where(rng.random(int(rem.sum())) < 0.5, 2.5, 2.6).astype(np.float32)
    final = (rng.random(n) < 0.3).astype(np.uint8)
    F = Forest(R, T, part, leaves, fl, final)
    api.depth_reset(g)
    api.set_depths_batch(g, R)
    per_tree = np.diff(F.first)[F.with_cells]
    a, b = loop_host(g, F), forest_host(g, F)                           # warm-up of each, and the comparison
    host_loop, host_forest, dev_forest = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        loop_host(g, F)
        host_loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        forest_host(g, F)
        host_forest.append(time.perf_counter() - t0)
    D = DeviceForm(g, F)
    D.forest()
    d = D.decisions()
    for _ in range(REPS):
        dev_forest.append(D.forest())
    reg = fl < 0
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "branches": int(len(bk)), "min_trees": MT, "subtrees": int(part.n_trees), "level": level, "cells": n,
           "subtrees_with_cells": len(F.with_cells),
           "cells_per_subtree": {"min": int(per_tree.min()), "median": float(np.median(per_tree)), "max": int(per_tree.max())},
           "regularized": int(reg.sum()), "removed": int(b[1].sum()), "split": int(b[2].sum()), "children": int(b[3].sum()),
           "regularize_constants": int(np.isin(b[0][reg], [np.float32(2.5), np.float32(2.6)]).sum()),
           "forest_equals_loop_decisions": {"host_pointers": bool(same(a, b)), "device_pointers": bool(same(a, d))},
           "host_pointers": {"per_tree_loop": spread(host_loop), "forest": spread(host_forest)},
           "device_pointers": {"forest": spread(dev_forest)}}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    del D
    g.close()
    # (c) the C++ levels, on a scene object of their own
    rec["cpp"] = cpp_levels(scene, F, T)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
