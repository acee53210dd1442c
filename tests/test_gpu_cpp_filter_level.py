"""The C++ host layer's PatchOptimizer::filterLevel / filterExtendLevel (tests/native/filter_level_cpp.cpp, built here with g++ against
libhpmvs_host.so) and hpmvs_amd.frontier's filter_level / filter_extend_level on the same dumped state: keep, dist, the losers, stage
codes, counts, accepted set, waves, occupancy, the refined candidates and every depth map are byte-identical, and the losers' images_
are cleared as the reference does (CellProcessor.cpp:72)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene
from test_gpu_filter_level import _grid_cells, _survivors, _width

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_filter_levels_equal_python(tiny_scene, gpu_scene, tmp_path):
    from hpmvs_amd import api, frontier
    exe = str(tmp_path / "filter_level_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "filter_level_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    R = _survivors(tiny_scene, gpu_scene, 400, 11)
    width = _width(R, 3.0)
    P, cs, occ0 = _grid_cells(R, width)
    n, nc = P.n, len(cs) - 1
    dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
    _dump_scene(dump, tiny_scene, P, n)
    with open(dump, "ab") as f:
        f.write(struct.pack("i", nc) + cs.astype(np.int32).tobytes() + struct.pack("fii", width, 0, len(occ0)))
        f.write(np.array(sorted(occ0), np.uint64).tobytes())
    r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    def maps_equal():
        for v in range(gpu_scene.n_views):
            for l in range(gpu_scene.view_levels[v]):
                rows, cols = take(np.int32, 2)
                d = take(np.float32, int(rows) * int(cols))
                if d.tobytes() != api.depth_level(gpu_scene, v, l).tobytes():
                    return False
        return True

    def fresh():
        api.depth_reset(gpu_scene)
        P.ok[:] = 1
        api.set_depths_batch(gpu_scene, P)

    # (A) filterLevel == filter_level
    fresh()
    F = frontier.filter_level(gpu_scene, P, cs)
    assert np.array_equal(take(np.int32, nc), F.keep) and take(np.float32, n).tobytes() == F.dist.tobytes()
    assert np.array_equal(take(np.uint8, n), F.removed)
    losers = int(F.removed.sum())
    assert int(take(np.int32, 1)[0]) == losers and losers >= 20
    assert maps_equal()
    # (B) filterExtendLevel == filter_extend_level
    fresh()
    occ = set(occ0)
    F, L = frontier.filter_extend_level(gpu_scene, P, cs, width, occ)
    assert np.array_equal(take(np.int32, nc), F.keep) and take(np.float32, n).tobytes() == F.dist.tobytes()
    assert np.array_equal(take(np.uint8, n), F.removed)
    st_py = np.where(np.isin(L.stage, (0, 20, 23, 24, 25, 26)), L.stage, 1)   # (C++ folds the refinement / gate failures into 1)
    assert np.array_equal(take(np.int32, 6 * nc), st_py) and np.array_equal(take(np.int32, 18 * nc).reshape(-1, 3), L.counts)
    A = int(take(np.int32, 1)[0])
    assert take(np.int32, A).tolist() == L.accepted
    assert int(take(np.int32, 1)[0]) == L.waves
    O = int(take(np.int32, 1)[0])
    assert take(np.uint64, O).tolist() == sorted(occ)
    assert take(np.float32, 24 * nc).tobytes() == L.candidates.center.tobytes()
    assert take(np.float32, 24 * nc).tobytes() == L.candidates.normal.tobytes()
    assert int(take(np.int32, 1)[0]) == losers
    assert maps_equal()
    assert off == len(buf)
    print("cpp filter level: rows", n, "cells", nc, "losers", losers, "accepted", A, "waves", L.waves)
    assert A >= 5
