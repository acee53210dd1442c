"""An extend level's wave walk at production size: the 50-view 4K scene, seed set and forest of tools/extend_forest_scale.py, the
98 304-candidate forest level.  Writes profiles/level_walk_scale.json and prints it as one JSON line.

  (a) the C++ forest level, PatchOptimizer::extendLevelForest (tests/native/bench_extend_level_forest, built here, on ONE dump of
      the scene) with HPMVS_LEVEL_TIMES=1, for three builds alternating cpp_reps times in fresh processes: the parent commit's
      build ($HPMVS_PARENT_LIBS names a folder with its libhpmvs_amd.so and libhpmvs_host.so; used through LD_LIBRARY_PATH), this
      build with the host walk, this build with HPMVS_DEVICE_WALK=1 (ONE hpmvs_level_walk_batch).  Median (min to max) of the
      line's "gates + walk + setDepths" and of the whole level, from the second pass of each run.
  (b) the Python level, frontier.extend_level_forest, with and without device_walk on that level from the same maps and trees: wall
      time, the results compared, the device call's waves and rounds.  py = 0 skips this part.

    python tools/level_walk_scale.py [views w h seeds leaves min_trees [cpp_reps [py]]]   (default: 50 3840 2160 100000 16384 100 5 1)"""
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

RECORD = os.path.join(ROOT, "profiles", "level_walk_scale.json")
SWITCHES = ("HPMVS_HOST_GRAPH", "HPMVS_DEVICE_GRAPH", "HPMVS_DEVICE_WALK")


def cpp_level(exe, dump, env):
    """One run of bench_extend_level_forest: the forest level's HPMVS_LEVEL_TIMES line of the second pass -> the times in ms."""
    saved = {k: os.environ.get(k) for k in list(env) + list(SWITCHES)}
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in env.items():
        os.environ[k] = v + ":" + saved[k] if k == "LD_LIBRARY_PATH" and saved[k] else v
    try:
        line = efs.cpp_run(exe, dump)["level_times"]["extendLevelForest"][-1]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    num = lambda what: float(re.search(what + r" ([0-9.]+) ms", line).group(1))
    parts = {k: num(k) for k in ("candidates' leaves", "refinement", "footprints", "conflict graph", "gates", "walk", "setDepths")}
    return {"waves_ms": round(parts["gates"] + parts["walk"] + parts["setDepths"], 1), "level_ms": round(sum(parts.values()), 1), "line": line}


def octrees(F):
    """The forest as frontier.extend_level_forest takes it: one Octree per subtree."""
    from hpmvs_amd import frontier
    trees = []
    for k in range(F.n_trees):
        bk, lk = F.keys_of(k)
        t = frontier.Octree(F.roots[k, :3], F.roots[k, 3])
        t.branches = {int(b) for b in bk}
        for i, key in enumerate(lk):
            t.leaves[int(key)] = i
            t._count(int(key), +1)
        trees.append(t)
    return trees


def python_level(g, R, F, device_walk):
    from hpmvs_amd import api, frontier
    api.depth_reset(g)
    R.ok[:] = 1
    api.set_depths_batch(g, R)
    trees = octrees(F)
    t0 = time.perf_counter()
    L = frontier.extend_level_forest(g, F.P, F.parent_tree, float(F.width), trees, device_walk=device_walk)
    return time.perf_counter() - t0, L


def main(argv):
    import torch
    from hpmvs_amd import api, frontier, synth
    V, W_, H_, NS, NL, MT = (int(a) for a in argv[:6]) if len(argv) >= 6 else (50, 3840, 2160, 100000, 16384, 100)
    cpp_reps = int(argv[6]) if len(argv) >= 7 else 5
    py = int(argv[7]) if len(argv) >= 8 else 1
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
    rec = {"scene": f"{V} x {W_}x{H_}", "build": api.build_id(), "candidates": 6 * P.n, "subtrees": int(F.n_trees)}
    if py:
        t_host, H = python_level(g, R, F, False)
        t_dev, D = python_level(g, R, F, True)
        rounds = api.last_level_walk(g)
        same = H.stage.tobytes() == D.stage.tobytes() and H.counts.tobytes() == D.counts.tobytes() and H.accepted == D.accepted and \
            H.waves == D.waves and H.deferred_per_wave == D.deferred_per_wave and H.border == D.border and H.leaf_key == D.leaf_key
        rec["python_extend_level_forest"] = {
            "host_walk_s": round(t_host, 3), "device_walk_s": round(t_dev, 3), "device_equals_host": bool(same), "refined": int((D.candidates.stage == 0).sum()),
            "accepted": len(D.accepted), "waves": D.waves, "deferred_per_wave": D.deferred_per_wave, "rounds": rounds[0],
            "most_rounds_in_a_wave": rounds[1], "in_order_passes": rounds[2]}
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1)
    g.close()
    runs = {"parent_build": [], "host_walk": [], "device_walk": []}
    parent = os.environ.get("HPMVS_PARENT_LIBS")
    if cpp_reps:
        exe = efs.cpp_build()
        dump = os.path.join(os.environ.get("TMPDIR", "/tmp"), "level_walk_scene.bin")
        efs.cpp_dump(scene, F, dump)
        try:
            for _ in range(cpp_reps):
                if parent:
                    runs["parent_build"].append(cpp_level(exe, dump, {"LD_LIBRARY_PATH": os.path.abspath(parent)}))
                runs["host_walk"].append(cpp_level(exe, dump, {}))
                runs["device_walk"].append(cpp_level(exe, dump, {"HPMVS_DEVICE_WALK": "1"}))
        finally:
            os.remove(dump)
    ms = lambda rs, k: efs.spread([1e-3 * r[k] for r in rs])
    rec["cpp_extendLevelForest"] = {k: {"gates_walk_setDepths": ms(v, "waves_ms"), "level": ms(v, "level_ms"), "last_line": v[-1]["line"]}
                                    for k, v in runs.items() if v}
    c = rec["cpp_extendLevelForest"]
    if "parent_build" in c and "device_walk" in c:
        p, d = c["parent_build"]["gates_walk_setDepths"], c["device_walk"]["gates_walk_setDepths"]
        rec["device_walk_below_parent_by_more_than_its_spread"] = bool(p["median_ms"] - d["median_ms"] > p["max_ms"] - p["min_ms"])
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
