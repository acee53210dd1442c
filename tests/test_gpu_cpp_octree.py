"""The C++ host layer's Scene::octreeLocate (tests/native/octree_locate_cpp.cpp, built here with g++ against libhpmvs_host.so) and
hpmvs_amd.api.octree_locate_batch on the same dumped tree and points: all six outputs are byte-identical, with and without
addWidth, and a tree that is none is refused."""
import os
import subprocess

import numpy as np
import pytest

import octree_tree_ref as otr
from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _tree():
    rng = np.random.default_rng(77)
    center, W = np.array([-1.0, 0.5, 3.0], f32), f32(6.0)
    T = otr.Tree(center, W)
    pts = (rng.uniform(-0.5, 0.5, (700, 3)) * float(W) + center).astype(f32)
    for i, p in enumerate(pts):
        T.add_at(p, i, f32(float(W) * 2.0 ** -rng.uniform(2, 9)))
    for i in rng.integers(0, len(pts), 60):
        T.remove(T.at(pts[i]))
    branches, leaves, _ = T.key_sets()
    points = np.concatenate([pts, (center + rng.uniform(-1.0, 1.0, (1300, 3)) * float(W)).astype(f32)])
    points[5, 1] = np.nan
    return center, W, np.array(sorted(branches), np.uint64), np.array(sorted(leaves), np.uint64), points, \
        (float(W) * 2.0 ** -rng.uniform(0, 10, len(points))).astype(f32)


def test_cpp_octree_locate_equals_python(tiny_scene, gpu_scene, tiny_seeds, tmp_path):
    from hpmvs_amd import api
    exe = str(tmp_path / "octree_locate_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "octree_locate_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    center, W, bk, lk, points, aw = _tree()
    n = len(points)
    for what, widths, leaf_keys, status in (("with addWidth", aw, lk, 0), ("without", None, lk, 0),
                                            ("a leaf twice", aw, np.concatenate([lk, lk[:1]]), 3)):
        dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
        _dump_scene(dump, tiny_scene, tiny_seeds, 0)
        with open(dump, "ab") as f:
            f.write(np.array(list(center) + [W], f32).tobytes())
            f.write(np.int32(len(bk)).tobytes() + bk.tobytes() + np.int32(len(leaf_keys)).tobytes() + leaf_keys.tobytes())
            f.write(np.int32(n).tobytes() + points.tobytes())
            f.write(np.int32(widths is not None).tobytes() + (b"" if widths is None else widths.tobytes()))
        if os.path.exists(outp):
            os.remove(outp)
        r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == status, (what, r.returncode, r.stderr)
        if status:
            assert "twice" in r.stderr and not os.path.exists(outp)
            continue
        want = api.octree_locate_batch(gpu_scene, center, W, bk, leaf_keys, points, widths)
        assert open(outp, "rb").read() == b"".join(getattr(want, name).tobytes() for name, _, _ in otr.OUTPUTS), what
        assert (want.leaf_index >= 0).sum() > 100 and (want.inside == 0).sum() > 100
        assert ((want.target_key != 0).sum() > 100) == (widths is not None)
