"""The C++ host layer with the conflict graph made on the device.  tests/native/extend_level_forest_cpp.cpp --
extendLevelTree, extendLevelForest and filterExtendLevelForest on the dumped state of tests/test_gpu_cpp_extend_level_forest.py --
runs in a fresh child process per setting: HPMVS_DEVICE_GRAPH=1 (hpmvs_level_conflicts_batch), HPMVS_HOST_GRAPH=1 and the
default (both build_conflict_graph from the footprints).  The outputs must be the same bytes: stages, counts, accepted, leaf keys, waves,
the candidates, keep / dist / removed, every tree and every depth-map cell.  The same for the grid-key caller filterExtendLevel
(tests/native/filter_level_cpp.cpp on the dumped state of tests/test_gpu_cpp_filter_level.py).  And Scene::levelConflicts
(tests/native/level_conflicts_cpp.cpp) equals hpmvs_amd.api.level_conflicts on the same patches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene
from test_gpu_extend_level_forest import K, MIN_SPLIT
from test_gpu_extend_level_tree import CASES, level_parents, make_seed_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    return exe


def _survivors(g, scene, c):
    from hpmvs_amd import api
    b = make_seed_batch(scene, c["groups"])
    api.optimize_batch(g, b)
    k = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
    R.ok[:] = 1
    return R


SETTINGS = (("device", {"HPMVS_DEVICE_GRAPH": "1"}), ("host", {"HPMVS_HOST_GRAPH": "1"}), ("default", {}))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("HPMVS_HOST_GRAPH", "HPMVS_DEVICE_GRAPH", "HPMVS_LEVEL_TIMES")}
    env.update(extra)
    return env


def test_levels_are_the_same_bytes_with_the_graph_from_the_host_and_from_the_device(tmp_path):
    from hpmvs_amd import api, frontier, synth
    from hpmvs_amd.frontier import key_depth
    exe = _build(tmp_path, "extend_level_forest_cpp")
    c = CASES["configs0"]
    scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        R = _survivors(g, scene, c)
        T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=False)     # (floors R.scale in place)
        O = frontier.Octree.from_seed_tree(T)
        P = frontier.partition(g, O, min_trees=K, min_split_leaves=MIN_SPLIT)
        levels = []
        for depth in sorted({key_depth(k) for k in O.leaves})[:2]:
            leaves, tree = [], []
            for t, S in enumerate(P.trees):
                d = depth - key_depth(int(P.root_key[t]))
                mine = level_parents(S, T, d)[1] if d >= 1 else []
                leaves += mine
                tree += [t] * len(mine)
            cells = [T.rows[T.cell_start[l]:T.cell_start[l + 1]] for l in leaves]
            levels.append(dict(width=np.float32(O.cell(next(k for k in O.leaves if key_depth(k) == depth))[1]),
                               parents=[int(T.rows[T.cell_start[l]]) for l in leaves], tree=np.array(tree, np.int32),
                               rows=np.concatenate(cells).astype(np.int32),
                               cs=np.concatenate([[0], np.cumsum([len(x) for x in cells])]).astype(np.int32)))
        one = int(levels[0]["tree"][len(levels[0]["tree"]) // 2])
        dump = tmp_path / "state.bin"
        _dump_scene(dump, scene, R, R.n)
        with open(dump, "ab") as f:
            f.write(struct.pack("i", len(P.trees)))
            for S in P.trees:
                bk, lk = S.branch_keys(), S.leaf_table()[0]
                f.write(np.array([*S.root_center, S.root_width], np.float32).tobytes())
                f.write(struct.pack("i", len(bk)) + bk.tobytes() + struct.pack("i", len(lk)) + lk.tobytes())
            for lv in levels:
                f.write(struct.pack("fi", float(lv["width"]), len(lv["parents"])) + np.array(lv["parents"], np.int32).tobytes())
                f.write(lv["tree"].tobytes() + lv["cs"].tobytes() + lv["rows"].tobytes())
            f.write(struct.pack("i", one))
    finally:
        g.close()
    out, err = {}, {}
    for name, extra in SETTINGS:
        outp = tmp_path / (name + ".bin")
        res = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600, env=_env(HPMVS_LEVEL_TIMES="1", **extra))
        assert res.returncode == 0, (name, res.stderr)
        out[name], err[name] = open(outp, "rb").read(), res.stderr
    assert len(out["host"]) > 1000
    assert out["device"] == out["host"], "the levels with the device graph differ from the levels with the host graph"
    assert out["default"] == out["host"]
    # the device run took the device call (its footprint step is part of the graph step: timed as 0), the host runs did not; all
    # report the same number of edges per level, and the levels have conflicts to get right
    import re
    edges = {name: re.findall(r"\((\d+) \+ (\d+) edges\)", err[name]) for name in err}
    assert edges["device"] == edges["host"] == edges["default"] and len(edges["host"]) >= 4, edges
    assert any(int(a) + int(b) > 0 for a, b in edges["host"]), edges
    assert "footprints 0.0 ms" in err["device"], err["device"]
    waves = {name: re.findall(r" wave (\d+):", err[name]) for name in err}
    assert waves["device"] == waves["host"] and len(waves["host"]) >= 4


def test_filter_extend_level_is_the_same_bytes_with_the_graph_from_the_host_and_from_the_device(tiny_scene, gpu_scene, tmp_path):
    """A grid-key caller with events: walk_level's branch without a tree (postKey from leafKey, the one shared occupied set)."""
    from test_gpu_filter_level import _grid_cells, _width
    from test_gpu_filter_level import _survivors as filter_survivors
    exe = _build(tmp_path, "filter_level_cpp")
    R = filter_survivors(tiny_scene, gpu_scene, 400, 11)      # the state of tests/test_gpu_cpp_filter_level.py
    width = _width(R, 3.0)
    P, cs, occ0 = _grid_cells(R, width)
    nc = len(cs) - 1
    dump = tmp_path / "state.bin"
    _dump_scene(dump, tiny_scene, P, P.n)
    with open(dump, "ab") as f:
        f.write(struct.pack("i", nc) + cs.astype(np.int32).tobytes() + struct.pack("fii", width, 0, len(occ0)))
        f.write(np.array(sorted(occ0), np.uint64).tobytes())
    out, err = {}, {}
    for name, extra in SETTINGS:
        outp = tmp_path / (name + ".bin")
        res = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600, env=_env(HPMVS_LEVEL_TIMES="1", **extra))
        assert res.returncode == 0, (name, res.stderr)
        out[name], err[name] = open(outp, "rb").read(), res.stderr
    # keep / dist / removed, stages, counts, accepted, waves, occupancy, the candidates and every depth-map cell, of both parts
    assert len(out["host"]) > 1000
    assert out["device"] == out["host"], "filterExtendLevel with the device graph differs from filterExtendLevel with the host graph"
    assert out["default"] == out["host"]
    import re
    edges = {name: re.findall(r"filterExtendLevel \d+ candidates.*\((\d+) \+ (\d+) edges\)", err[name]) for name in err}
    assert edges["device"] == edges["host"] == edges["default"] and len(edges["host"]) == 1, (edges, err["host"])
    assert all(int(a) + int(b) > 0 for a, b in edges["host"]), edges
    assert "footprints 0.0 ms" in err["device"], err["device"]
    waves = {name: re.findall(r"filterExtendLevel wave (\d+):", err[name]) for name in err}
    assert waves["device"] == waves["host"] and len(waves["host"]) >= 1, waves


def test_scene_level_conflicts_equals_the_binding(tmp_path):
    from hpmvs_amd import api, synth
    exe = _build(tmp_path, "level_conflicts_cpp")
    c = CASES["configs0"]
    scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        R = _survivors(g, scene, c)
        n = R.n
        is_ev = (np.arange(n) % 3 == 2).astype(np.uint8)
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
        _dump_scene(dump, scene, R, n)
        with open(dump, "ab") as f:
            f.write(is_ev.tobytes())
        res = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600, env=_env())
        assert res.returncode == 0, res.stderr
        buf, off = open(outp, "rb").read(), 0

        def take(count):
            nonlocal off
            a = np.frombuffer(buf, dtype=np.uint32, count=count, offset=off)
            off += a.nbytes
            return a

        api.depth_reset(g)
        api.set_depths_batch(g, R)
        for ev in (None, is_ev):
            fo, fa, ao, aa = api.level_conflicts(g, R, ev)
            assert len(fa) + len(aa) > 0
            assert int(take(1)[0]) == len(fa) and take(n + 1).tobytes() == fo.tobytes() and take(len(fa)).tobytes() == fa.tobytes()
            assert int(take(1)[0]) == len(aa) and take(n + 1).tobytes() == ao.tobytes() and take(len(aa)).tobytes() == aa.tobytes()
        assert take(4).tolist() == [0, 0, 0, 0]   # n == 0: no edges, flowOff = antiOff = [0]
        assert off == len(buf)
    finally:
        g.close()
