"""The C++ host layer's Scene::octreePartition (tests/native/octree_partition_cpp.cpp, built here with g++ against
libhpmvs_host.so) and hpmvs_amd.api.octree_partition on the same dumped tree: every output is byte-identical, with the reference's
defaults and with a small threshold, and a tree that is none is refused."""
import os
import subprocess

import numpy as np
import pytest

import octree_partition_ref as opr
from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_cpp_octree_partition_equals_python(tiny_scene, gpu_scene, tiny_seeds, tmp_path):
    from hpmvs_amd import api
    exe = str(tmp_path / "octree_partition_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "octree_partition_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    center, W, bk, lk = opr.tree("random")
    for what, leaf_keys, min_trees, min_split, status in (("the defaults", lk, 100, 100, 0), ("a small threshold", lk, 1000, 3, 0),
                                                          ("the root alone", lk, 1, 100, 0),
                                                          ("a leaf twice", np.concatenate([lk, lk[:1]]), 100, 100, 3)):
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
        _dump_scene(dump, tiny_scene, tiny_seeds, 0)
        with open(dump, "ab") as f:
            f.write(np.array(list(center) + [W], f32).tobytes())
            f.write(np.int32(len(bk)).tobytes() + bk.tobytes() + np.int32(len(leaf_keys)).tobytes() + leaf_keys.tobytes())
            f.write(np.int32(min_trees).tobytes() + np.int32(min_split).tobytes())
        if os.path.exists(outp):
            os.remove(outp)
        r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == status, (what, r.returncode, r.stderr)
        if status:
            assert "twice" in r.stderr and not os.path.exists(outp)
            continue
        P = api.octree_partition(gpu_scene, center, W, bk, leaf_keys, min_trees, min_split)
        n = P.n_trees
        want = np.array([n, P.n_orphans, P.n_splits, P.stop], np.int32).tobytes() + P.histogram.tobytes()
        want += P.root_key[:n].tobytes() + P.root_cell[:n].tobytes() + P.tree_first[:n].tobytes() + P.tree_leaves[:n].tobytes()
        want += b"".join(getattr(P, name).tobytes() for name in api.PARTITION_OUTPUTS[4:])
        assert open(outp, "rb").read() == want, what
        assert (n > 8 if min_trees > 1 else n == 1) and P.tree_leaves[:n].sum() + P.n_orphans == len(lk)
