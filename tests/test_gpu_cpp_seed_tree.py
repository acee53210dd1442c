"""The C++ host layer's Scene::seedTree (tests/native/seed_tree_cpp.cpp, built here with g++ against libhpmvs_host.so) and
hpmvs_amd.frontier's seed_tree on the same dumped patches: root, floor, every scale_3dx_, the leaf tables and every depth map are
byte-identical."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("maxlevel", [9, 3])
def test_cpp_seed_tree_equals_python(tiny_scene, gpu_scene, tmp_path, maxlevel):
    from hpmvs_amd import api, frontier, synth
    exe = str(tmp_path / "seed_tree_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "seed_tree_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    seeds = synth.make_seeds(tiny_scene, 500, start_level=2, seed=synth.SEED + 23)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gpu_scene, b)
    keep = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[keep], b.normal[keep], b.scale[keep], b.n_images[keep], b.images[keep])
    R.ok[:] = 1
    n = R.n
    assert n > 100
    dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
    _dump_scene(dump, tiny_scene, R, n)
    with open(dump, "ab") as f:
        f.write(np.int32(maxlevel).tobytes())
    r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    api.depth_reset(gpu_scene)
    t = frontier.seed_tree(gpu_scene, R, patch_init_maxlevel=maxlevel, set_depths=True)
    root = take(np.float32, 5)
    assert root.tobytes() == np.array(list(t.root_center) + [t.root_width, t.scale_floor], np.float32).tobytes()
    assert take(np.float32, n).tobytes() == R.scale.tobytes()
    nr, L = (int(x) for x in take(np.int32, 2))
    assert nr == n == len(t.rows) and L == t.n_leaves
    assert np.array_equal(take(np.int32, nr), t.rows) and np.array_equal(take(np.int32, L + 1), t.cell_start)
    assert take(np.float32, 3 * L).tobytes() == t.cell_center.tobytes() and take(np.float32, L).tobytes() == t.cell_width.tobytes()
    assert np.array_equal(take(np.int32, L), t.cell_level) and take(np.float32, 3 * L).tobytes() == t.patch_center.tobytes()
    for v in range(tiny_scene.n_views):
        for l in range(gpu_scene.view_levels[v]):
            rows, cols = (int(x) for x in take(np.int32, 2))
            assert take(np.float32, rows * cols).tobytes() == api.depth_level(gpu_scene, v, l).tobytes()
    assert off == len(buf)
    print("cpp seed tree: maxlevel", maxlevel, "rows", n, "leaves", L, "largest cell", int(np.diff(t.cell_start).max()))
