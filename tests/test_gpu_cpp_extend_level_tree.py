"""The C++ host layer's PatchOptimizer::extendLevelTree / filterExtendLevelTree (tests/native/extend_level_tree_cpp.cpp, built here
with g++ against libhpmvs_host.so) and hpmvs_amd.frontier's extend_level_tree / filter_extend_level_tree on the same dumped state:
BASELINE configs[0] through seed_tree, the whole tree and the subtree root of tests/test_gpu_extend_level_tree.py.  (A) the two
lowest populated levels in turn, the index carried from the first to the second; (B) from a fresh state the first level with its
filter, and then the second (the coarsest level's leaves hold one patch each: the losers are on the next).  Equal: stage codes (C++ folds refinement and gate failures into 1), counts, accepted order, border list, leaf keys, waves,
the final branch and leaf key sets, the candidates' centre and normal bytes, keep / dist / removed, the losers' cleared images_, and
every depth map."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene
from test_gpu_extend_level_tree import CASES, level_parents, make_seed_batch, subtree_root, two_lowest_levels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1.0


def test_cpp_tree_levels_equal_python(tmp_path):
    from hpmvs_amd import api, frontier, synth
    exe = str(tmp_path / "extend_level_tree_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "extend_level_tree_cpp.cpp"), "-o", exe,
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

        def tree_of(whole):
            root = subtree_root(O, 0 if whole else c["sub_depth"])
            return O.subtree(root) if root != 1 else frontier.Octree.from_seed_tree(T)

        runs = []
        for whole in (True, False):
            S = tree_of(whole)
            levels = []
            for depth in two_lowest_levels(S):
                keys, leaves = level_parents(S, T, depth)
                cells = [T.rows[T.cell_start[l]:T.cell_start[l + 1]] for l in leaves]
                levels.append(dict(width=np.float32(S.cell(keys[0])[1]), parents=[int(T.rows[T.cell_start[l]]) for l in leaves],
                                   rows=np.concatenate(cells).astype(np.int32),
                                   cs=np.concatenate([[0], np.cumsum([len(x) for x in cells])]).astype(np.int32)))
            runs.append(dict(whole=whole, levels=levels))
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
        _dump_scene(dump, scene, R, R.n)
        with open(dump, "ab") as f:
            f.write(struct.pack("i", len(runs)))
            for r in runs:
                S = tree_of(r["whole"])
                bk, lk = S.branch_keys(), S.leaf_table()[0]
                f.write(np.array([*S.root_center, S.root_width], np.float32).tobytes())
                f.write(struct.pack("i", len(bk)) + bk.tobytes() + struct.pack("i", len(lk)) + lk.tobytes())
                for lv in r["levels"]:
                    f.write(struct.pack("fi", float(lv["width"]), len(lv["parents"])) + np.array(lv["parents"], np.int32).tobytes())
                    f.write(lv["cs"].tobytes() + lv["rows"].tobytes())
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
        for r in runs:
            what = "whole" if r["whole"] else "subtree"
            # (A) extendLevelTree == extend_level_tree, level after level on one tree
            fresh()
            S = tree_of(r["whole"])
            for i, lv in enumerate(r["levels"]):
                L = frontier.extend_level_tree(g, frontier._rows(R, lv["parents"]), lv["width"], S, MARGIN, 0)
                level_equal(L, (what, "level", i))
            tree_equal(S, (what, "tree after two levels"))
            assert maps_equal(), (what, "maps after two levels")
            # (B) filterExtendLevelTree == filter_extend_level_tree
            fresh()
            S = tree_of(r["whole"])
            for i, lv in enumerate(r["levels"]):
                n, nc = len(lv["rows"]), len(lv["cs"]) - 1
                F, L = frontier.filter_extend_level_tree(g, frontier._rows(R, lv["rows"]), lv["cs"], lv["width"], S, margin=MARGIN, abs_int=0)
                assert np.array_equal(take(np.int32, nc), F.keep) and take(np.float32, n).tobytes() == F.dist.tobytes(), (what, i)
                assert np.array_equal(take(np.uint8, n), F.removed), (what, i)
                level_equal(L, (what, "filter level", i))
                losers = int(F.removed.sum())
                assert int(take(np.int32, 1)[0]) == losers, (what, i, "the losers' images_ are cleared")
                tally["losers"] += losers
            tree_equal(S, (what, "tree after the filter levels"))
            assert maps_equal(), (what, "maps after the filter levels")
        assert off == len(buf)
        print("cpp extend_level_tree:", tally)
        assert tally["stage26"] >= 1 and tally["stage27"] >= 1 and tally["accepted"] >= 5 and tally["losers"] >= 5, tally
    finally:
        g.close()
