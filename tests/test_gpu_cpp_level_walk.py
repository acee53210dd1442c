"""The C++ host layer with the waves of a level walked on the device.  tests/native/extend_level_forest_cpp.cpp --
extendLevelTree, extendLevelForest and filterExtendLevelForest on the dumped state of tests/test_gpu_cpp_level_conflicts.py -- and
tests/native/filter_level_cpp.cpp -- the grid-key caller filterExtendLevel -- each run in a fresh child process with and without
HPMVS_DEVICE_WALK=1 (ONE hpmvs_level_walk_batch per level against walk_level's own loop).  The outputs must be the same bytes:
stages, counts, accepted, leaf keys, waves, the candidates, keep / dist / removed, every tree and every depth-map cell."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene
from test_gpu_cpp_level_conflicts import _build, _survivors
from test_gpu_extend_level_forest import K, MIN_SPLIT
from test_gpu_extend_level_tree import CASES, level_parents

pytestmark = pytest.mark.gpu
SETTINGS = (("device", {"HPMVS_DEVICE_WALK": "1"}), ("host", {}))
SWITCHES = ("HPMVS_HOST_GRAPH", "HPMVS_DEVICE_GRAPH", "HPMVS_DEVICE_WALK", "HPMVS_LEVEL_TIMES")


def _run_both(exe, dump, tmp_path):
    out, err = {}, {}
    for name, extra in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(HPMVS_LEVEL_TIMES="1", **extra)
        outp = tmp_path / (name + ".bin")
        res = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, (name, res.stderr)
        out[name], err[name] = open(outp, "rb").read(), res.stderr
    return out, err


def _checks(out, err, levels):
    assert len(out["host"]) > 1000
    assert out["device"] == out["host"], "the levels walked on the device differ from the levels walked on the host"
    # the host run walked its waves here (a line per wave, more than one wave on some level); the device run made none of them and
    # its summary lines carry the call under "walk"
    assert len(re.findall(r" wave (\d+):", err["host"])) > levels and not re.findall(r" wave (\d+):", err["device"]), err["device"]
    lines = re.findall(r"waves: gates ([0-9.]+) ms, walk ([0-9.]+) ms, setDepths ([0-9.]+) ms", err["device"])
    assert len(lines) == levels and all(g == "0.0" and s == "0.0" for g, _, s in lines), err["device"]
    assert len(re.findall(r"waves: gates", err["host"])) == levels


def test_forest_levels_are_the_same_bytes_walked_on_the_host_and_on_the_device(tmp_path):
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
    out, err = _run_both(exe, dump, tmp_path)
    _checks(out, err, len(re.findall(r"waves: gates", err["host"])))
    assert len(re.findall(r"waves: gates", err["host"])) >= 4


def test_filter_extend_level_is_the_same_bytes_walked_on_the_host_and_on_the_device(tiny_scene, gpu_scene, tmp_path):
    """A grid-key caller with events: one set, the caller's occupied set grows by the accepted leaves."""
    from test_gpu_filter_level import _grid_cells, _width
    from test_gpu_filter_level import _survivors as filter_survivors
    exe = _build(tmp_path, "filter_level_cpp")
    R = filter_survivors(tiny_scene, gpu_scene, 400, 11)
    width = _width(R, 3.0)
    P, cs, occ0 = _grid_cells(R, width)
    dump = tmp_path / "state.bin"
    _dump_scene(dump, tiny_scene, P, P.n)
    with open(dump, "ab") as f:
        f.write(struct.pack("i", len(cs) - 1) + cs.astype(np.int32).tobytes() + struct.pack("fii", width, 0, len(occ0)))
        f.write(np.array(sorted(occ0), np.uint64).tobytes())
    out, err = _run_both(exe, dump, tmp_path)
    _checks(out, err, 1)
