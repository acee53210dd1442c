"""One extend level against the real octree at production size: the leaves of the most populated level of the 50-view 4K scene's
seed tree (up to 16 384 parents = 98 304 candidates).  Writes profiles/extend_level_tree_scale.json and prints it as one JSON line.

  (a) hpmvs_extend_tree_batch against the four calls it replaces -- hpmvs_expand_batch with everything skipped,
      hpmvs_octree_locate_batch, hpmvs_expand_batch, hpmvs_octree_locate_batch, with the centres reshaped between them -- on the
      same inputs in one process, with host pointers and with device pointers: after one warm-up of each the two forms alternate
      REPS times, wall clock around calls that end synchronised; medians and the spread (min, max) of each.  The outputs of the
      two are compared byte for byte once.
  (b) the C++ host layer's PatchOptimizer::extendLevelTree beside extendLevel (grid keys) on the same parents
      (tests/native/bench_extend_level_tree.cpp, built here), with the HPMVS_LEVEL_TIMES breakdown of both.

    python tools/extend_level_tree_scale.py [views w h seeds leaves]        (default: 50 3840 2160 100000 16384)
    python tools/extend_level_tree_scale.py --calls-only [views w h seeds leaves]   the device-pointer fused call alone, three
                                                                        times: run THIS under `rocprofv3 --kernel-trace --stats`"""
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

RECORD = os.path.join(ROOT, "profiles", "extend_level_tree_scale.json")
REPS = 5
KEYS = (("skip", np.uint8), ("pre_inside", np.uint8), ("pre_key", np.uint64), ("border", np.uint8), ("post_key", np.uint64))


def spread(ts):
    ms = [1e3 * t for t in ts]
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def four_calls_host(g, P, width, T, bk, lk):
    from hpmvs_amd import api
    n = P.n
    cc, cw = np.zeros((n, 3), np.float32), np.full(n, width, np.float32)
    aw = np.float32(float(width) * 0.9)
    pre = api.expand_batch(g, api.EXPAND_EXTEND, P, cc, cw, np.ones(6 * n, np.uint8))
    a = api.octree_locate_batch(g, T.root_center, T.root_width, bk, lk, pre.center, aw)
    inside = a.inside != 0
    skip = (inside & ((a.leaf_index >= 0) | (a.leaf_width < width))).astype(np.uint8)
    out = api.expand_batch(g, api.EXPAND_EXTEND, P, cc, cw, skip)
    b = api.octree_locate_batch(g, T.root_center, T.root_width, bk, lk, out.center, aw)
    ok = out.ok != 0
    border = ok & (b.inside == 0)
    return out, dict(skip=skip, pre_inside=a.inside, pre_key=a.target_key * inside.astype(np.uint64), border=border.astype(np.uint8),
                     post_key=b.target_key * (ok & ~border).astype(np.uint64))


class DeviceForm:
    """The same inputs on the device: the parents, the keys, an out batch, the key arrays and the look-ups' outputs."""

    def __init__(self, g, P, width, T, bk, lk):
        import torch
        from hpmvs_amd import api
        self.torch, self.api, self.g, self.width = torch, api, g, np.float32(width)
        self.n, N = P.n, 6 * P.n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.keep = {k: up(getattr(P, k)) for k in api.Batch.FIELDS}
        self.pb = api.PatchBatch()
        self.pb.n, self.pb.max_images = P.n, P.max_images
        for k, v in self.keep.items():
            setattr(self.pb, k, v.data_ptr())
        blank = api.Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                          np.zeros((N, P.max_images), np.int32))
        self.out = {k: up(getattr(blank, k)) for k in api.Batch.FIELDS}
        self.ob = api.PatchBatch()
        self.ob.n, self.ob.max_images = N, P.max_images
        for k, v in self.out.items():
            setattr(self.ob, k, v.data_ptr())
        self.center = self.out["center"].view(torch.float32).view(N, 4)
        self.tb, self.tl = up(bk), up(lk)
        self.t = api.OctreeIndex()
        for k in range(3):
            self.t.root_center[k] = float(T.root_center[k])
        self.t.root_width = float(T.root_width)
        self.t.n_branches, self.t.n_leaves = len(bk), len(lk)
        self.t.branch_key, self.t.leaf_key = self.tb.data_ptr(), self.tl.data_ptr()
        self.cc, self.cw = torch.zeros(3 * P.n, dtype=torch.float32, device="cuda"), torch.full((P.n,), float(width), dtype=torch.float32, device="cuda")
        self.aw = torch.full((N,), float(np.float32(float(width) * 0.9)), dtype=torch.float32, device="cuda")
        self.ones = torch.ones(N, dtype=torch.uint8, device="cuda")
        self.inside = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.index = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.lwidth = torch.zeros(N, dtype=torch.float32, device="cuda")
        self.target = torch.zeros(N, dtype=torch.int64, device="cuda")
        self.keys = {k: torch.zeros(N * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for k, dt in KEYS}
        self.kb = api.ExtendTreeKeysStruct()
        for k, v in self.keys.items():
            setattr(self.kb, k, v.data_ptr())
        self.o = api.default_options()
        torch.cuda.synchronize()

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.api.lib().hpmvs_last_error().decode())

    def _expand(self, skip):
        self._chk(self.api.lib().hpmvs_expand_batch(self.g.h, C.byref(self.o), 0, C.byref(self.pb), self.cc.data_ptr(), self.cw.data_ptr(),
                                                    skip.data_ptr(), C.byref(self.ob), 1, None))

    def _locate(self):
        pts = self.center[:, :3].contiguous()          # [n][4] -> [n][3]
        self._chk(self.api.lib().hpmvs_octree_locate_batch(self.g.h, C.byref(self.t), 6 * self.n, pts.data_ptr(), self.aw.data_ptr(),
                                                           self.inside.data_ptr(), None, self.index.data_ptr(), self.lwidth.data_ptr(), None,
                                                           self.target.data_ptr(), 1, None))

    def four_calls(self):
        t0 = time.perf_counter()
        self._expand(self.ones)
        self._locate()
        skip = ((self.inside != 0) & ((self.index >= 0) | (self.lwidth < float(self.width)))).to(self.torch.uint8)
        self._expand(skip)
        self._locate()
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0

    def fused(self):
        t0 = time.perf_counter()
        self._chk(self.api.lib().hpmvs_extend_tree_batch(self.g.h, C.byref(self.o), C.byref(self.t), C.byref(self.pb), float(self.width),
                                                         C.byref(self.ob), C.byref(self.kb), 1, None))
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0


def cpp_levels(scene, P, width, T, bk, lk):
    """(b): tests/native/bench_extend_level_tree on the same parents; -> its JSON line and the HPMVS_LEVEL_TIMES lines."""
    exe = os.path.join(ROOT, "tests", "native", "bench_extend_level_tree")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, exe + ".cpp", "-o", exe, "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd",
                    "-Wl,-rpath," + lib], check=True)
    dump = os.path.join(os.environ.get("TMPDIR", "/tmp"), "extend_level_tree_scene.bin")
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
        f.write(struct.pack("f", float(width)) + np.array([*T.root_center, T.root_width], np.float32).tobytes())
        f.write(struct.pack("i", len(bk)) + bk.tobytes() + struct.pack("i", len(lk)) + lk.tobytes())
    try:
        r = subprocess.run([exe, dump], capture_output=True, text=True, env=dict(os.environ, HPMVS_LEVEL_TIMES="1"))
    finally:
        os.remove(dump)
    if r.returncode != 0:
        raise SystemExit(f"bench_extend_level_tree failed: {r.stdout}\n{r.stderr}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    # the second pass of each (the first warms the pinned-memory cache and the workspaces)
    lines = [l for l in r.stderr.splitlines() if l.startswith("extendLevel") and "candidates (" in l]
    rec["level_times"] = {"extendLevel": [l for l in lines if l.startswith("extendLevel ")][-1:],
                          "extendLevelTree": [l for l in lines if l.startswith("extendLevelTree ")][-1:]}
    return rec


def main(argv):
    import torch
    from hpmvs_amd import api, frontier, synth
    calls_only = bool(argv) and argv[0] == "--calls-only"
    if calls_only:
        argv = argv[1:]
    V, W_, H_, NS, NL = (int(a) for a in argv[:5]) if len(argv) >= 5 else (50, 3840, 2160, 100000, 16384)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    if T.n_leaves == 0:
        raise SystemExit(f"no seed survived on {V} x {W_}x{H_}: take a larger scene")
    bk, lk = path_keys(T)
    level = int(np.bincount(T.cell_level).argmax())                  # the most populated level: its leaves are the parents
    leaves = np.nonzero(T.cell_level == level)[0][:NL]
    P = frontier._rows(R, T.rows[T.cell_start[leaves]])
    width = np.float32(T.cell_width[leaves[0]])
    D = DeviceForm(g, P, width, T, bk, lk)
    if calls_only:
        for _ in range(3):
            D.fused()
        print(json.dumps({"calls_only": True, "candidates": 6 * P.n}))
        return None
    # (a) host pointers
    want, wkeys = four_calls_host(g, P, width, T, bk, lk)            # warm-up of each, and the comparison
    out, k = api.extend_tree_batch(g, P, width, T.root_center, T.root_width, bk, lk)
    same = all(getattr(out, f).tobytes() == getattr(want, f).tobytes() for f in api.Batch.FIELDS) and \
        all(getattr(k, f).tobytes() == wkeys[f].tobytes() for f, _ in KEYS)
    host4, host1, dev4, dev1 = [], [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        four_calls_host(g, P, width, T, bk, lk)
        host4.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        api.extend_tree_batch(g, P, width, T.root_center, T.root_width, bk, lk)
        host1.append(time.perf_counter() - t0)
    # device pointers
    D.four_calls(); D.fused()
    for _ in range(REPS):
        dev4.append(D.four_calls())
        dev1.append(D.fused())
    refined = k.skip == 0
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "seeds": NS, "survivors": R.n, "leaves": int(T.n_leaves),
           "branches": int(len(bk)), "level": level, "width": float(width), "parents": P.n, "candidates": 6 * P.n,
           "pre_gated": int(k.skip.sum()), "outside_before_optimize": int((k.pre_inside == 0).sum()), "refined_ok": int(out.ok.sum()),
           "border": int(k.border.sum()), "refused_after_optimize": int(((out.ok != 0) & (k.border == 0) & (k.post_key == 0)).sum()),
           "not_pre_gated": int(refined.sum()), "fused_equals_four_calls_bytes": bool(same),
           "host_pointers": {"four_calls": spread(host4), "fused": spread(host1)},
           "device_pointers": {"four_calls": spread(dev4), "fused": spread(dev1)}}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    g.close()
    # (b) the C++ levels, on a scene object of their own
    rec["cpp"] = cpp_levels(scene, P, width, T, bk, lk)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
