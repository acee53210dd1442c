"""The C++ host layer's --only_sphere (tests/native/scene_center_cpp.cpp, built here with g++ against libhpmvs_host.so):
Scene::getSceneCenter, Scene::initPatches with options.FILTER_SCENE_CENTER and the overload with an explicit sphere, on the
configs[0] model of test_gpu_nvm_files.py read from files, against the same calls through hpmvs_amd.api.  Bytes, no tolerances.

The model gets three extra points p_i = c_i + 2.2 (centre - c_i), one behind the scene centre on every camera's line to it, each
measured in all three views: 36 from the centre against a radius of 30, and inside all three START_LEVEL-2 images with the
margin, so un-gated they reach optimize()."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_nvm_files import write_nvm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Reader:
    def __init__(self, buf):
        self.buf, self.off = buf, 0

    def take(self, dtype, count=1):
        a = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.off)
        self.off += a.nbytes
        return a

    def run(self):
        ok = int(self.take(np.int32)[0])
        stage = self.take(np.int32, int(self.take(np.int32)[0]))
        patches = []
        for _ in range(int(self.take(np.int32)[0])):
            f = self.take(np.float32, 13)
            patches.append((f, self.take(np.int32, int(self.take(np.int32)[0]))))
        return ok, stage, patches


def survivors(batch):
    """the rows Scene::initPatches returns, as scene_center_cpp writes them"""
    out = []
    for k in np.nonzero(batch.ok)[0]:
        f = np.concatenate([batch.center[k], batch.normal[k], [batch.scale[k], batch.ncc[k]], batch.color[k]]).astype(np.float32)
        out.append((f, batch.images[k, :batch.n_images[k]]))
    return out


def same_patches(a, b):
    return len(a) == len(b) and all(fa.tobytes() == fb.tobytes() and np.array_equal(ia, ib) for (fa, ia), (fb, ib) in zip(a, b))


def test_cpp_only_sphere_equals_python(tiny_scene, gpu_scene, tmp_path):
    from hpmvs_amd import api, synth
    exe = str(tmp_path / "scene_center_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "scene_center_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    centre, radius = api.scene_center(gpu_scene.cameras)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 300, start_level=2, noise=1.0)
    extra = np.array([v.c + 2.2 * (centre - v.c) for v in tiny_scene.views])
    n0, n = len(xyz), len(xyz) + len(extra)
    xyz = np.concatenate([xyz, extra])
    off = np.concatenate([off, off[-1] + 3 * np.arange(1, len(extra) + 1)]).astype(np.int32)
    img = np.concatenate([img, np.tile(np.arange(3, dtype=np.int32), len(extra))]).astype(np.int32)
    dist = np.linalg.norm(xyz - centre, axis=1)
    assert (dist[:n0] < radius - 1.0).all() and np.allclose(dist[n0:], 36.0, atol=1e-3) and abs(radius - 30.0) < 1e-3

    for i, v in enumerate(tiny_scene.views):
        with open(tmp_path / ("view%02d.ppm" % i), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (v.width, v.height) + np.ascontiguousarray(v.rgb).tobytes())
    nvm, outp = tmp_path / "scene.nvm", tmp_path / "out.bin"
    write_nvm(nvm, tiny_scene, xyz, off, img)
    r = subprocess.run([exe, str(nvm), str(outp), "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rd = Reader(open(outp, "rb").read())

    # getSceneCenter returns the C ABI's doubles
    assert int(rd.take(np.int32)[0]) == 1
    assert rd.take(np.float64, 3).tobytes() == centre.tobytes() and rd.take(np.float64)[0] == radius

    plain = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, max_images=64)
    assert not np.isin(plain.stage[n0:], (10, 11, 13, 100)).any()  # un-gated, the extra points reach optimize()
    small = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, max_images=64, sphere=(0.0, 0.0, 0.0, 5.0))
    own = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, max_images=64, sphere=(*centre, radius))
    assert 0 < small.ok.sum() < own.ok.sum() and (small.stage == 13).sum() > 3

    # the explicit overload at (0, 0, 0; 5): Python's survivors, order and fields, and its stage vector
    ok, stage, patches = rd.run()
    assert ok == 1 and np.array_equal(stage, small.stage) and same_patches(patches, survivors(small))
    # FILTER_SCENE_CENTER = true is the explicit overload at getSceneCenter's values
    ok, stage, filtered = rd.run()
    assert ok == 1 and len(stage) == 0
    ok, stage, explicit = rd.run()
    assert ok == 1 and same_patches(filtered, explicit) and same_patches(explicit, survivors(own))
    assert np.array_equal(stage, own.stage)
    assert np.array_equal(np.nonzero(stage == 13)[0], np.arange(n0, n))  # exactly the three extra points
    # FILTER_SCENE_CENTER = false: today's output
    ok, stage, unfiltered = rd.run()
    assert ok == 1 and len(stage) == 0 and same_patches(unfiltered, survivors(plain))
    assert rd.off == len(rd.buf)
    print("cpp only_sphere: survivors", len(patches), "at (0,0,0;5),", len(filtered), "in the scene sphere,", len(unfiltered),
          "un-gated; un-gated stages of the extra points", plain.stage[n0:])
