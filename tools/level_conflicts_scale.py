"""An extend level's conflict graph at production size: the 50-view 4K scene, seed set and forest of tools/extend_forest_scale.py,
the refined candidates of the most populated level (98 304 candidates by default) as the graph's nodes.  Writes
profiles/level_conflicts_scale.json and prints it as one JSON line.

  (a) the device call alone, hpmvs_level_conflicts_batch with host pointers (api.level_conflicts: no footprint leaves the device),
      against what the C++ walk does on the host: hpmvs_depth_footprints_batch to the host, then clear_event_reads /
      build_conflict_graph / add_event_edges (the hook hpmvs_host_conflict_graph of libhpmvs_host.so, OpenMP as in walk_level).
      After one warm-up of each the two alternate REPS times in one process; medians and the spread (min, max).  The two graphs
      are compared byte for byte (the host lists sorted).
  (b) the C++ forest level, PatchOptimizer::extendLevelForest (tests/native/bench_extend_level_forest, built here) with
      HPMVS_LEVEL_TIMES=1: this build with HPMVS_DEVICE_GRAPH=1, this build with HPMVS_HOST_GRAPH=1 and, when $HPMVS_PARENT_LIBS names a
      folder with libhpmvs_amd.so and libhpmvs_host.so of the parent commit, that build (through LD_LIBRARY_PATH), alternating
      cpp_reps times in fresh processes; "footprints + conflict graph" and the whole level from the second pass of each run (the
      first warms the pinned-memory cache and the workspaces).  cpp_reps = 0 skips this part.

    python tools/level_conflicts_scale.py [views w h seeds leaves min_trees [cpp_reps]]   (default: 50 3840 2160 100000 16384 100 5)"""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import extend_forest_scale as efs  # noqa: E402
from octree_locate_scale import path_keys, seed_tree  # noqa: E402

RECORD = os.path.join(ROOT, "profiles", "level_conflicts_scale.json")
REPS = 5


def host_graph(L, nodes, fp, n_levels, max_w, max_h):
    wr, fr, at, vb = fp
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    fo, ao = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    fa, aa = np.zeros(64 * n, np.uint32), np.zeros(64 * n, np.uint32)
    nf, na = C.c_uint32(0), C.c_uint32(0)
    ni = np.ascontiguousarray(nodes.n_images, np.int32)
    rc = L.hpmvs_host_conflict_graph(n, M, V, n_levels, max_w, max_h, ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data,
                                     vb.ctypes.data, None, fo.ctypes.data, fa.ctypes.data, fa.size, ao.ctypes.data, aa.ctypes.data, aa.size,
                                     C.byref(nf), C.byref(na))
    if rc != 0:
        raise SystemExit(f"hpmvs_host_conflict_graph: {rc}")
    return fo, fa[:nf.value], ao, aa[:na.value]


def cpp_level(scene, F, env):
    """One run of bench_extend_level_forest: the forest level's HPMVS_LEVEL_TIMES line of the second pass -> the times in ms."""
    os.environ.pop("HPMVS_HOST_GRAPH", None)
    os.environ.pop("HPMVS_DEVICE_GRAPH", None)
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ[k] = v + ":" + saved[k] if k == "LD_LIBRARY_PATH" and saved[k] else v
    try:
        line = efs.cpp_levels(scene, F)["level_times"]["extendLevelForest"][-1]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    num = lambda what: float(re.search(what + r" ([0-9.]+) ms", line).group(1))
    parts = {k: num(k) for k in ("candidates' leaves", "refinement", "footprints", "conflict graph", "gates", "walk", "setDepths")}
    return {"footprints_plus_graph_ms": round(parts["footprints"] + parts["conflict graph"], 1), "level_ms": round(sum(parts.values()), 1),
            "edges": re.search(r"\((\d+ \+ \d+) edges\)", line).group(1), "line": line}


def main(argv):
    import torch
    from hpmvs_amd import api, frontier, synth
    V, W_, H_, NS, NL, MT = (int(a) for a in argv[:6]) if len(argv) >= 6 else (50, 3840, 2160, 100000, 16384, 100)
    cpp_reps = int(argv[6]) if len(argv) >= 7 else 5
    scene = synth.make_scene(V, W_, H_, n_waves=24, device=torch.device("cuda", 0))
    g = api.Scene(scene)
    R, T = seed_tree(g, scene, V, NS)
    if T.n_leaves == 0:
        raise SystemExit(f"no seed survived on {V} x {W_}x{H_}: take a larger scene")
    bk, lk = path_keys(T)
    part = api.octree_partition(g, T.root_center, T.root_width, bk, lk, min_trees=MT)
    level = int(np.bincount(T.cell_level).argmax())
    leaves = np.nonzero((T.cell_level == level) & (part.leaf_tree >= 0))[0][:NL]
    leaves = leaves[np.argsort(part.leaf_tree[leaves], kind="stable")]
    P = frontier._rows(R, T.rows[T.cell_start[leaves]])
    F = efs.Forest(T, bk, lk, part, P, part.leaf_tree[leaves], T.cell_width[leaves[0]])
    api.depth_reset(g)
    R.ok[:] = 1
    api.set_depths_batch(g, R)
    out, keys = efs.forest_host(g, F)
    refined = np.nonzero((out.stage == 0) & (keys.skip == 0))[0]
    nodes = frontier._rows(out, refined)
    n_levels = frontier._pyramid_levels(g, "level_conflicts_scale")
    L = C.CDLL(os.path.join(ROOT, "hpmvs_amd", "libhpmvs_host.so"))
    L.hpmvs_host_conflict_graph.argtypes = [C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    # (a) warm-up of each and the comparison, then the alternation
    dev = api.level_conflicts(g, nodes)
    host = host_graph(L, nodes, api.depth_footprints_batch(g, nodes), n_levels, W_, H_)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(dev, host))
    t_dev, t_fp, t_build = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        api.level_conflicts(g, nodes)
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        fp = api.depth_footprints_batch(g, nodes)
        t1 = time.perf_counter()
        host_graph(L, nodes, fp, n_levels, W_, H_)
        t_fp.append(t1 - t0); t_build.append(time.perf_counter() - t1)
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "candidates": 6 * P.n, "nodes": int(nodes.n), "max_images": int(nodes.max_images),
           "pyramid_levels": n_levels, "flow_edges": int(len(dev[1])), "anti_edges": int(len(dev[3])),
           "device_equals_host_bytes": bool(same),
           "device_call": efs.spread(t_dev), "host_footprints": efs.spread(t_fp), "host_build": efs.spread(t_build),
           "host_footprints_plus_build": efs.spread([a + b for a, b in zip(t_fp, t_build)]),
           "footprint_words_per_node": int(11 * nodes.max_images + 3 * V)}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    g.close()
    # (b) the C++ forest level, host graph and device graph alternating in fresh processes
    runs = {"parent_build": [], "host_graph": [], "device_graph": []}
    parent = os.environ.get("HPMVS_PARENT_LIBS")
    for _ in range(cpp_reps):
        if parent:
            runs["parent_build"].append(cpp_level(scene, F, {"LD_LIBRARY_PATH": os.path.abspath(parent)}))
        runs["host_graph"].append(cpp_level(scene, F, {"HPMVS_HOST_GRAPH": "1"}))
        runs["device_graph"].append(cpp_level(scene, F, {"HPMVS_DEVICE_GRAPH": "1"}))
    ms = lambda rs, k: efs.spread([1e-3 * r[k] for r in rs])
    rec["cpp_extendLevelForest"] = {k: {"footprints_plus_graph": ms(v, "footprints_plus_graph_ms"), "level": ms(v, "level_ms"),
                                        "edges": v[-1]["edges"], "last_line": v[-1]["line"]} for k, v in runs.items() if v}
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
