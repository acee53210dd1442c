"""The C++ host layer's PatchOptimizer::extendLevelForest / filterExtendLevelForest (tests/native/extend_level_forest_cpp.cpp,
built here with g++ against libhpmvs_host.so) and hpmvs_amd.frontier's extend_level_forest / filter_extend_level_forest on the same
dumped state: BASELINE configs[0] through seed_tree and the partition of tests/test_gpu_extend_level_forest.py.  The extend level
over the lowest populated node level, then the filter level over the second with the forest carried on.  Equal: stage codes (C++
folds refinement and gate failures into 1), counts, accepted order, border list, leaf keys, every candidate's tree, waves, every
tree's branch and leaf key sets, the candidates' centre and normal bytes, keep / dist / removed, the losers' cleared images_, and
every depth map.  Before and after the forest levels the program runs extendLevelTree on one tree alone: both runs equal
frontier.extend_level_tree, and LevelResult::tree stays empty there."""
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
MARGIN = 1.0


def test_cpp_forest_levels_equal_python(tmp_path):
    import copy
    from hpmvs_amd import api, frontier, synth
    from hpmvs_amd.frontier import key_depth
    exe = str(tmp_path / "extend_level_forest_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "extend_level_forest_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    c = CASES["configs0"]
    scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        b = make_seed_batch(scene, c["groups"])
        api.optimize_batch(g, b)
        k = np.nonzero(b.ok)[0]
        R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
        R.ok[:] = 1
        T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=False)     # (floors R.scale in place)
        assert sorted(T.rows.tolist()) == list(range(R.n))
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
        assert len(np.unique(levels[0]["tree"])) >= 3
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
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
        res = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        buf = open(outp, "rb").read()
        off = 0

        def take(dtype, count):
            nonlocal off
            a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
            off += a.nbytes
            return a

        def maps_equal():
            same = True
            for v in range(g.n_views):
                for l in range(g.view_levels[v]):
                    rows, cols = take(np.int32, 2)
                    same &= take(np.float32, int(rows) * int(cols)).tobytes() == api.depth_level(g, v, l).tobytes()
            return same

        def fresh():
            api.depth_reset(g)
            R.ok[:] = 1
            api.set_depths_batch(g, R)

        def level_equal(L, what):
            N = L.candidates.n
            st_py = np.where(np.isin(L.stage, (0, 20, 23, 24, 25, 26, 27)), L.stage, 1)   # (C++ folds the refinement / gate failures into 1)
            st = take(np.int32, N)
            assert np.array_equal(st, st_py), (what, np.nonzero(st != st_py)[0][:8])
            assert np.array_equal(take(np.int32, 3 * N).reshape(-1, 3), L.counts), what
            A = int(take(np.int32, 1)[0])
            assert take(np.int32, A).tolist() == L.accepted, what
            assert take(np.uint64, A).tolist() == [L.leaf_key[t] for t in L.accepted], what
            B = int(take(np.int32, 1)[0])
            assert take(np.int32, B).tolist() == L.border, what
            assert int(take(np.int32, 1)[0]) == L.waves, what
            assert take(np.float32, 4 * N).tobytes() == L.candidates.center.tobytes(), what
            assert take(np.float32, 4 * N).tobytes() == L.candidates.normal.tobytes(), what
            nt = int(take(np.int32, 1)[0])
            assert nt == len(L.tree) and np.array_equal(take(np.int32, nt), L.tree), what
            tally["accepted"] += A
            tally["stage26"] += int((L.stage == 26).sum())
            tally["stage27"] += int((L.stage == 27).sum())

        def tree_equal(S, what):
            nb = int(take(np.int32, 1)[0])
            bk = take(np.uint64, nb).tolist()
            nl = int(take(np.int32, 1)[0])
            lk = take(np.uint64, nl).tolist()
            assert len(set(bk)) == nb and len(set(lk)) == nl, what
            assert set(bk) == S.branches and set(lk) == set(S.leaves), what

        tally = dict(accepted=0, stage26=0, stage27=0, losers=0)

        def one_tree(what):
            fresh()
            S = copy.deepcopy(P.trees[one])
            lv = levels[0]
            L = frontier.extend_level_tree(g, frontier._rows(R, np.array(lv["parents"])[lv["tree"] == one]), lv["width"], S, MARGIN, 0)
            assert len(L.tree) == 0
            start = off
            level_equal(L, what)
            tree_equal(S, what)
            return buf[start:off]

        before = one_tree("extendLevelTree before the forest levels")
        fresh()
        trees = copy.deepcopy(P.trees)
        lv = levels[0]
        L = frontier.extend_level_forest(g, frontier._rows(R, lv["parents"]), lv["tree"], lv["width"], trees, MARGIN, 0)
        level_equal(L, "extendLevelForest")
        lv = levels[1]
        n, nc = len(lv["rows"]), len(lv["cs"]) - 1
        F, L = frontier.filter_extend_level_forest(g, frontier._rows(R, lv["rows"]), lv["cs"], lv["tree"], lv["width"], trees, margin=MARGIN,
                                                   abs_int=0)
        assert np.array_equal(take(np.int32, nc), F.keep) and take(np.float32, n).tobytes() == F.dist.tobytes()
        assert np.array_equal(take(np.uint8, n), F.removed)
        level_equal(L, "filterExtendLevelForest")
        losers = int(F.removed.sum())
        assert int(take(np.int32, 1)[0]) == losers, "the losers' images_ are cleared"
        tally["losers"] += losers
        for t, S in enumerate(trees):
            tree_equal(S, ("tree", t, "after the forest levels"))
        assert maps_equal(), "maps after the forest levels"
        after = one_tree("extendLevelTree after the forest levels")
        assert before == after
        assert off == len(buf)
        print("cpp extend_level_forest:", tally, "trees", len(trees))
        assert tally["stage26"] >= 1 and tally["stage27"] >= 1 and tally["accepted"] >= 5 and tally["losers"] >= 5, tally
    finally:
        g.close()
