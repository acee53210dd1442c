"""One extend level over the subtrees of main's getSubTrees at production size: the 50-view 4K scene and seed set of
tools/extend_level_tree_scale.py, the seed tree cut by hpmvs_octree_partition(min_trees=100), the parents of the most populated
level (up to 16 384 = 98 304 candidates) grouped by subtree.  Writes profiles/extend_forest_scale.json and prints it as one JSON
line.

  (a) the loop a scheduler that follows main makes today: ONE hpmvs_extend_tree_batch per subtree that has parents;
  (b) ONE hpmvs_extend_forest_batch over all of them.
      Both on the same inputs in one process, with host pointers and with device pointers: after one warm-up of each the two
      alternate REPS times, wall clock around calls that end synchronised; medians and the spread (min, max) of each.  The outputs
      of the two are compared byte for byte once.  (a) is the baseline: the same code the parent commit has.
  (c) the C++ host layer: the per-tree loop of PatchOptimizer::extendLevelTree beside ONE extendLevelForest on the same parents
      (tests/native/bench_extend_level_forest.cpp, built here), with the HPMVS_LEVEL_TIMES breakdown of both.

    python tools/extend_forest_scale.py [views w h seeds leaves min_trees]        (default: 50 3840 2160 100000 16384 100)"""
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

RECORD = os.path.join(ROOT, "profiles", "extend_forest_scale.json")
REPS = 5
KEYS = (("skip", np.uint8), ("pre_inside", np.uint8), ("pre_key", np.uint64), ("border", np.uint8), ("post_key", np.uint64))


def spread(ts):
    ms = [1e3 * t for t in ts]
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


class Forest:
    """The subtrees as the calls take them, and the parents grouped by subtree (parent_tree non-decreasing)."""

    def __init__(self, T, bk, lk, part, P, parent_tree, width):
        n = part.n_trees
        self.n_trees, self.width, self.P, self.parent_tree = n, np.float32(width), P, np.ascontiguousarray(parent_tree, np.int32)
        self.roots = np.ascontiguousarray(part.root_cell[:n], np.float32)
        border, lorder = np.argsort(part.branch_tree, kind="stable"), np.argsort(part.leaf_tree, kind="stable")
        border, lorder = border[part.branch_tree[border] >= 0], lorder[part.leaf_tree[lorder] >= 0]
        self.branch_key, self.leaf_key = part.branch_sub_key[border].copy(), part.leaf_sub_key[lorder].copy()
        self.branch_first = np.searchsorted(part.branch_tree[border], np.arange(n + 1)).astype(np.int32)
        self.leaf_first = np.searchsorted(part.leaf_tree[lorder], np.arange(n + 1)).astype(np.int32)
        self.first = np.searchsorted(self.parent_tree, np.arange(n + 1)).astype(np.int64)     # tree k's parents: first[k] .. first[k + 1] - 1
        self.with_parents = [k for k in range(n) if self.first[k + 1] > self.first[k]]
        from hpmvs_amd import frontier
        self.parents_of = {k: frontier._rows(P, np.arange(self.first[k], self.first[k + 1])) for k in self.with_parents}

    def keys_of(self, k):
        return (self.branch_key[self.branch_first[k]:self.branch_first[k + 1]], self.leaf_key[self.leaf_first[k]:self.leaf_first[k + 1]])


def loop_host(g, F):
    """(a) with host pointers -> the rows of all trees, in the parents' order."""
    from hpmvs_amd import api
    outs = []
    for k in F.with_parents:
        bk, lk = F.keys_of(k)
        outs.append(api.extend_tree_batch(g, F.parents_of[k], F.width, F.roots[k, :3], F.roots[k, 3], bk, lk))
    return outs


def forest_host(g, F):
    from hpmvs_amd import api
    return api.extend_forest_batch(g, F.P, F.parent_tree, F.width, F.roots, F.branch_first, F.leaf_first, F.branch_key, F.leaf_key)


class DeviceForm:
    """The same inputs on the device.  The parents are grouped by tree, so tree k's share of every array is one slice: the loop
    hands hpmvs_extend_tree_batch pointers into the buffers the forest call takes whole."""

    def __init__(self, g, F):
        import torch
        from hpmvs_amd import api
        self.torch, self.api, self.g, self.F = torch, api, g, F
        P = F.P
        N = 6 * P.n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.par = {k: up(getattr(P, k)) for k in api.Batch.FIELDS}
        blank = api.Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                          np.zeros((N, P.max_images), np.int32))
        self.out = {k: up(getattr(blank, k)) for k in api.Batch.FIELDS}
        self.row_bytes = {k: getattr(blank, k).nbytes // max(N, 1) for k in api.Batch.FIELDS}
        self.keys = {k: torch.zeros(N * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for k, dt in KEYS}
        self.tb, self.tl, self.pt = up(F.branch_key), up(F.leaf_key), up(F.parent_tree)
        self.o = api.default_options()
        self.f = api.OctreeForest()
        self.f.n_trees = F.n_trees
        self.f.root, self.f.branch_first, self.f.leaf_first = F.roots.ctypes.data, F.branch_first.ctypes.data, F.leaf_first.ctypes.data
        self.f.branch_key, self.f.leaf_key = self.tb.data_ptr(), self.tl.data_ptr()
        self.pb, self.ob, self.kb = self._batches(0, P.n)
        self.per_tree = []
        for k in F.with_parents:
            t = api.OctreeIndex()
            for c in range(3):
                t.root_center[c] = float(F.roots[k, c])
            t.root_width = float(F.roots[k, 3])
            t.n_branches, t.n_leaves = int(F.branch_first[k + 1] - F.branch_first[k]), int(F.leaf_first[k + 1] - F.leaf_first[k])
            t.branch_key = self.tb.data_ptr() + 8 * int(F.branch_first[k]) if t.n_branches else None
            t.leaf_key = self.tl.data_ptr() + 8 * int(F.leaf_first[k]) if t.n_leaves else None
            self.per_tree.append((t,) + self._batches(int(F.first[k]), int(F.first[k + 1])))
        torch.cuda.synchronize()

    def _batches(self, a, b):
        """PatchBatch of the parents a .. b - 1, the out batch and the key struct of their candidates."""
        api, P = self.api, self.F.P
        pb, ob = api.PatchBatch(), api.PatchBatch()
        pb.n, pb.max_images, ob.n, ob.max_images = b - a, P.max_images, 6 * (b - a), P.max_images
        for k in api.Batch.FIELDS:
            setattr(pb, k, self.par[k].data_ptr() + a * (getattr(P, k).nbytes // max(P.n, 1)))
            setattr(ob, k, self.out[k].data_ptr() + 6 * a * self.row_bytes[k])
        kb = api.ExtendTreeKeysStruct()
        for k, dt in KEYS:
            setattr(kb, k, self.keys[k].data_ptr() + 6 * a * np.dtype(dt).itemsize)
        return pb, ob, kb

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.api.lib().hpmvs_last_error().decode())

    def loop(self):
        t0 = time.perf_counter()
        for t, pb, ob, kb in self.per_tree:
            self._chk(self.api.lib().hpmvs_extend_tree_batch(self.g.h, C.byref(self.o), C.byref(t), C.byref(pb), float(self.F.width), C.byref(ob),
                                                             C.byref(kb), 1, None))
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0

    def forest(self):
        t0 = time.perf_counter()
        self._chk(self.api.lib().hpmvs_extend_forest_batch(self.g.h, C.byref(self.o), C.byref(self.f), C.byref(self.pb), self.pt.data_ptr(),
                                                           float(self.F.width), C.byref(self.ob), C.byref(self.kb), 1, None))
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0

    def snapshot(self):
        self.torch.cuda.synchronize()
        return b"".join(v.cpu().numpy().tobytes() for v in list(self.out.values()) + list(self.keys.values()))


def cpp_build():
    """tests/native/bench_extend_level_forest, built here -> its path"""
    exe = os.path.join(ROOT, "tests", "native", "bench_extend_level_forest")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, exe + ".cpp", "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd",
                    "-Wl,-rpath," + lib], check=True)
    return exe


def cpp_dump(scene, F, dump):
    """The scene, the parents and the forest as bench_extend_level_forest reads them."""
    P = F.P
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
        f.write(struct.pack("f", float(F.width)) + F.parent_tree.tobytes() + struct.pack("i", F.n_trees))
        for k in range(F.n_trees):
            bk, lk = F.keys_of(k)
            f.write(F.roots[k].tobytes() + struct.pack("i", len(bk)) + bk.tobytes() + struct.pack("i", len(lk)) + lk.tobytes())


def cpp_run(exe, dump):
    """One run of bench_extend_level_forest on a dump, with the environment as it stands -> its JSON line and the HPMVS_LEVEL_TIMES lines."""
    r = subprocess.run([exe, dump], capture_output=True, text=True, env=dict(os.environ, HPMVS_LEVEL_TIMES="1"))
    if r.returncode != 0:
        raise SystemExit(f"bench_extend_level_forest failed: {r.stdout}\n{r.stderr}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    # the second pass of each (the first warms the pinned-memory cache and the workspaces): the forest's line, and of the loop's
    # lines of that pass the three largest subtrees'
    lines = [l for l in r.stderr.splitlines() if "candidates (" in l]
    loop = [l for l in lines if l.startswith("extendLevelTree ")]
    loop = loop[len(loop) // 2:]
    rec["level_times"] = {"extendLevelForest": [l for l in lines if l.startswith("extendLevelForest ")][-1:],
                          "extendLevelTree_largest": sorted(loop, key=lambda l: -int(l.split()[1]))[:3], "extendLevelTree_lines": len(loop)}
    return rec


def cpp_levels(scene, F):
    """(c): tests/native/bench_extend_level_forest on the same parents; -> its JSON line and the HPMVS_LEVEL_TIMES lines."""
    exe = cpp_build()
    dump = os.path.join(os.environ.get("TMPDIR", "/tmp"), "extend_forest_scene.bin")
    cpp_dump(scene, F, dump)
    try:
        return cpp_run(exe, dump)
    finally:
        os.remove(dump)


def main(argv):
    import torch
    from hpmvs_amd import api, frontier, synth
    V, W_, H_, NS, NL, MT = (int(a) for a in argv[:6]) if len(argv) >= 6 else (50, 3840, 2160, 100000, 16384, 100)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    if T.n_leaves == 0:
        raise SystemExit(f"no seed survived on {V} x {W_}x{H_}: take a larger scene")
    bk, lk = path_keys(T)
    part = api.octree_partition(g, T.root_center, T.root_width, bk, lk, min_trees=MT)
    level = int(np.bincount(T.cell_level).argmax())                  # the most populated level: its leaves are the parents
    leaves = np.nonzero((T.cell_level == level) & (part.leaf_tree >= 0))[0][:NL]
    leaves = leaves[np.argsort(part.leaf_tree[leaves], kind="stable")]     # the trees' queues one after the other
    P = frontier._rows(R, T.rows[T.cell_start[leaves]])
    F = Forest(T, bk, lk, part, P, part.leaf_tree[leaves], T.cell_width[leaves[0]])
    per_tree = np.diff(F.first)[F.with_parents]
    # host pointers: warm-up of each, and the comparison
    a, (out, keys) = loop_host(g, F), forest_host(g, F)
    same = all(np.concatenate([getattr(o, f) for o, _ in a]).tobytes() == getattr(out, f).tobytes() for f in api.Batch.FIELDS) and \
        all(np.concatenate([getattr(k, f) for _, k in a]).tobytes() == getattr(keys, f).tobytes() for f, _ in KEYS)
    host_loop, host_forest, dev_loop, dev_forest = [], [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        loop_host(g, F)
        host_loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        forest_host(g, F)
        host_forest.append(time.perf_counter() - t0)
    D = DeviceForm(g, F)
    D.loop()
    snap = D.snapshot()
    D.forest()
    same_dev = snap == D.snapshot()
    for _ in range(REPS):
        dev_loop.append(D.loop())
        dev_forest.append(D.forest())
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "branches": int(len(bk)), "min_trees": MT, "subtrees": int(part.n_trees), "orphans": int(part.n_orphans), "level": level,
           "width": float(F.width), "parents": P.n, "candidates": 6 * P.n, "subtrees_with_parents": len(F.with_parents),
           "candidates_per_subtree": {"min": int(6 * per_tree.min()), "median": float(6 * np.median(per_tree)), "max": int(6 * per_tree.max())},
           "pre_gated": int(keys.skip.sum()), "refined_ok": int(out.ok.sum()), "border": int(keys.border.sum()),
           "forest_equals_loop_bytes": {"host_pointers": bool(same), "device_pointers": bool(same_dev)},
           "host_pointers": {"per_tree_loop": spread(host_loop), "forest": spread(host_forest)},
           "device_pointers": {"per_tree_loop": spread(dev_loop), "forest": spread(dev_forest)}}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    del D
    g.close()
    # (c) the C++ levels, on a scene object of their own
    rec["cpp"] = cpp_levels(scene, F)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
