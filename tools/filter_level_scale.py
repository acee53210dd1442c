"""CellProcessor::filter (reference CellProcessor.cpp:43-82) at production size: the initial tree of Scene::initPatches
(Scene.cpp:183-199: root from the survivors' bounding box, DynOctTree::add(p, max(scale, width / 2^(PATCH_INIT_MAXLEVEL + 1))),
restated by tests/octree_ref.py) built from the seed loop's survivors on the 50-view 4K scene; its cell-size histogram; one
hpmvs_filter_batch over every nonempty leaf (host pointers, wall time of the call) against the host restatement in
tools/filter_host.cpp on 16 threads, keep compared cell by cell.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels'
own times.  Prints one JSON line.

    python tools/filter_level_scale.py [views w h seeds]      (default: 50 3840 2160 100000)

filterExtendLevel at 16 384 leaves (against the sequential CPU loop and against extendLevel on the same leaves reduced to one patch
each) is not part of this tool: those figures are recorded as "not measured"."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hpmvs_amd import api, synth  # noqa: E402
import octree_ref as ot  # noqa: E402

PATCH_INIT_MAXLEVEL = 9


def main(argv):
    V, W_, H_, NS = (int(a) for a in argv[:4]) if len(argv) >= 4 else (50, 3840, 2160, 100000)
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    seeds = synth.make_seeds(scene, NS, start_level=4, max_images=min(V, api.MAX_IMAGES))
    b0 = api.Batch.from_seeds(seeds)
    api.optimize_batch(g, b0)
    ok = np.nonzero(b0.ok)[0]
    P = b0.center[ok, :3].astype(np.float32)
    lo, hi = P.min(axis=0), P.max(axis=0)
    width = np.float32(max(hi - lo))
    tree = ot.OctTree(((lo + hi) / np.float32(2)).astype(np.float32), width, P)
    t0 = time.perf_counter()
    floor = np.float32(width / np.float32(1 << (PATCH_INIT_MAXLEVEL + 1)))
    for e in range(len(ok)):
        tree.add(e, max(np.float32(b0.scale[ok[e]]), floor))
    t_tree = time.perf_counter() - t0
    leaves = tree.nonempty()
    sizes = np.array([len(l.data) for l in leaves])
    rows = np.array([ok[e] for l in leaves for e in l.data])
    cs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cells = api.Batch(b0.center[rows], b0.normal[rows], b0.scale[rows], b0.n_images[rows], b0.images[rows])
    api.filter_batch(g, cells, cs)                               # warm-up
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dist, keep = api.filter_batch(g, cells, cs)
        walls.append(time.perf_counter() - t0)
    src = os.path.join(ROOT, "tools", "filter_host.cpp")
    so = os.path.join(tempfile.mkdtemp(), "libfilter_host.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fopenmp", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so], check=True)
    H = C.CDLL(so)
    H.filter_host.restype = C.c_double
    H.filter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    hd, hk = np.zeros(cells.n, np.float32), np.zeros(len(sizes), np.int32)
    host = [H.filter_host(cells.center.ctypes.data, cells.normal.ctypes.data, cs.ctypes.data, len(sizes), 16, hd.ctypes.data,
                          hk.ctypes.data) for _ in range(3)]
    hist = {str(int(k)): int(v) for k, v in zip(*np.unique(sizes, return_counts=True))}
    out = {"scene": f"{V} x {W_}x{H_}", "build": api.lib().hpmvs_build_id().decode(), "seeds": NS, "survivors": int(len(ok)),
           "tree_s_python_restatement": round(t_tree, 2), "leaves": int(len(sizes)), "rows": int(cells.n),
           "multi_patch_leaves": int((sizes > 1).sum()), "rows_in_multi_patch_leaves": int(sizes[sizes > 1].sum()),
           "largest_leaf": int(sizes.max()), "cell_size_histogram": hist,
           "filter_batch_call_ms_median": round(1e3 * float(np.median(walls)), 3),
           "host_restatement_16_threads_ms_median": round(1e3 * float(np.median(host)), 3),
           "keep_equal": bool(np.array_equal(keep, hk)), "dist_equal_bits": bool(dist.tobytes() == hd.tobytes()),
           "filter_extend_level_16384_leaves": "not measured", "sequential_cpu_loop_16384_leaves": "not measured",
           "extend_level_single_patch_16384_leaves": "not measured"}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
