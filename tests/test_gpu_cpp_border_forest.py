"""The C++ host layer's Scene::octreeBorderForest and PatchOptimizer::deliverBorderForest (tests/native/border_forest_cpp.cpp, built
here with g++ against libhpmvs_host.so) and hpmvs_amd.api.border_forest_batch on the same dumped forest and border queue -- the
special forest of tests/border_forest_ref.py with a queue of 2 000: every output is byte-identical, the accepted patches come back
with flatness_ 0 and the others untouched, the forest holds the accepted keys as OctreeIndex::insertLeaf enters them in queue
order, and a malformed forest is refused."""
import os
import subprocess

import numpy as np
import pytest

import border_forest_ref as bfr
from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _insert_leaf(branches, leaves, key):
    """OctreeIndex::insertLeaf on ordered lists"""
    leaves.append(key)
    k = key >> 3
    while k > 1:
        if k not in branches:
            branches.append(k)
        k >>= 3


def test_cpp_border_forest_equals_python(tiny_scene, tmp_path):
    from hpmvs_amd import api
    exe = str(tmp_path / "border_forest_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "border_forest_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    trees, center, scale = bfr.special_case(2000)
    n = len(scale)
    queue = api.Batch(center, np.zeros((n, 4), f32), scale, np.zeros(n, np.int32), np.full((n, 1), -1, np.int32))
    twice = list(trees)
    twice[4] = (trees[4][0], trees[4][1], np.concatenate([trees[4][2], trees[4][2][:1]]))
    g = api.Scene(tiny_scene, device=0)
    try:
        api.depth_reset(g)
        for what, forest, status in (("a round", trees, 0), ("a leaf twice", twice, 3)):
            roots, bf, lf, bk, lk = bfr.flatten(forest)
            dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
            _dump_scene(dump, tiny_scene, queue, n)
            with open(dump, "ab") as f:
                f.write(np.int32(len(forest)).tobytes() + roots.tobytes() + bf.tobytes() + lf.tobytes() + bk.tobytes() + lk.tobytes())
            if os.path.exists(outp):
                os.remove(outp)
            r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=300)
            assert r.returncode == status, (what, r.returncode, r.stderr)
            if status:
                assert "tree 4" in r.stderr and "twice" in r.stderr and not os.path.exists(outp)
                continue
            want = api.border_forest_batch(g, queue, roots, bf, lf, bk, lk, set_depths=True)
            four = want.tree.tobytes() + want.accepted.tobytes() + want.leaf_key.tobytes() + want.blocker.tobytes()
            flatness = np.where(want.accepted != 0, f32(0), f32(-1)).astype(f32)
            keys = b""
            for k, (_, tb, tl) in enumerate(forest):
                branches, leaves = [int(x) for x in tb], [int(x) for x in tl]
                for i in np.nonzero((want.accepted != 0) & (want.tree == k))[0]:
                    _insert_leaf(branches, leaves, int(want.leaf_key[i]))
                keys += np.int32(len(branches)).tobytes() + np.array(branches, np.uint64).tobytes()
                keys += np.int32(len(leaves)).tobytes() + np.array(leaves, np.uint64).tobytes()
            assert open(outp, "rb").read() == four + four + flatness.tobytes() + keys, what
            assert want.accepted.sum() > 100 and (want.blocker >= 0).sum() > 100 and (want.tree < 0).sum() > 50
            assert len(set(want.tree[want.accepted != 0].tolist())) >= 5
    finally:
        g.close()
