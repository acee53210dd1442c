"""The C++ host layer's Scene::octreeInsert and Scene::octreeRoute (tests/native/octree_insert_cpp.cpp, built here with g++ against
libhpmvs_host.so) and hpmvs_amd.api.octree_insert_batch / octree_route_batch on the same dumped tree, patches and roots: every
output is byte-identical, and a tree that is none and a root without width are refused."""
import os
import subprocess

import numpy as np
import pytest

import octree_insert_ref as oir
from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_cpp_octree_insert_and_route_equal_python(tiny_scene, gpu_scene, tiny_seeds, tmp_path):
    from hpmvs_amd import api
    exe = str(tmp_path / "octree_insert_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "octree_insert_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    (center, W, bk, lk), points, aw = oir.case("chain", 2000)
    rng = np.random.default_rng(9)
    roots, _ = oir.route_case(rng, 12, 0)
    roots[:, :3] = roots[:, :3] / f32(4) + center              # around the tree: some of its points fall into them
    no_width = roots.copy()
    no_width[3, 3] = 0
    for what, leaf_keys, rts, status in (("a round", lk, roots, 0), ("a leaf twice", np.concatenate([lk, lk[:1]]), roots, 3),
                                         ("a root without width", lk, no_width, 4)):
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
        _dump_scene(dump, tiny_scene, tiny_seeds, 0)
        with open(dump, "ab") as f:
            f.write(np.array(list(center) + [W], f32).tobytes())
            f.write(np.int32(len(bk)).tobytes() + bk.tobytes() + np.int32(len(leaf_keys)).tobytes() + leaf_keys.tobytes())
            f.write(np.int32(len(points)).tobytes() + points.tobytes() + aw.tobytes())
            f.write(np.int32(len(rts)).tobytes() + rts.tobytes())
        if os.path.exists(outp):
            os.remove(outp)
        r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == status, (what, r.returncode, r.stderr)
        if status:
            assert ("twice" if status == 3 else "positive width") in r.stderr and not os.path.exists(outp)
            continue
        want = api.octree_insert_batch(gpu_scene, center, W, bk, leaf_keys, points, aw)
        to = api.octree_route_batch(gpu_scene, rts, points)
        assert open(outp, "rb").read() == want.accepted.tobytes() + want.leaf_key.tobytes() + want.blocker.tobytes() + to.tobytes(), what
        assert want.accepted.sum() > 100 and (want.blocker >= 0).sum() > 100 and ((want.accepted == 0) & (want.blocker < 0)).sum() > 100
        assert (to >= 0).sum() > 50 and (to < 0).sum() > 50
