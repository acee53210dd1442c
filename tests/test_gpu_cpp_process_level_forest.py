"""The C++ host layer's PatchOptimizer::processLevelForest and OctreeIndex::applySweep (tests/native/process_level_forest_cpp.cpp,
built here with g++ against libhpmvs_host.so) and hpmvs_amd.frontier.process_level_forest on the same dumped state: BASELINE
configs[0] with the outliers, the partition and the drawn flatness of tests/test_gpu_process_level_forest.py.  Byte-identical:
flatness, neighbour counts, support, removed / split / children, child keys, the candidates' centres and normals, every tree's
branch and leaf key sets after the sweep with data[0]'s centre per leaf, and the depth maps behind the gates.  The C++ call resets
priorityReduction_ of the regularized cells only and clears images_ of removed and split cells only; a decreasing cellTree is
refused (the program checks that itself)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_interface import _dump_scene
from test_gpu_extend_level_tree import _state
from test_gpu_process_level_forest import _forest, _restore, _start, _started

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _state.values():
        s["g"].close()
    _state.clear()
    _started.clear()


def test_cpp_forest_sweep_equals_python(tmp_path):
    from hpmvs_amd import api, frontier
    exe = str(tmp_path / "process_level_forest_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "process_level_forest_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    s = _start("configs0")
    g, cells, ct, ck, fl, final, R, T = s["g"], s["cells"], s["ct"], s["ck"], s["fl"], s["final"], s["R"], s["T"]
    n = cells.n
    dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
    _dump_scene(dump, s["scene"], cells, n)
    trees = s["P"].trees
    with open(dump, "ab") as f:
        for i in range(n):
            f.write(np.float32(fl[i]).tobytes() + np.int32(ct[i]).tobytes() + np.uint64(ck[i]).tobytes() + np.uint8(final[i]).tobytes())
        rows = [int(r) for r in T.rows]
        f.write(struct.pack("i", len(rows)))
        for k in rows:
            m = int(R.n_images[k])
            f.write(R.center[k].tobytes() + R.normal[k].tobytes() + struct.pack("fi", float(R.scale[k]), m) + struct.pack(f"{m}i", *R.images[k, :m]))
        f.write(struct.pack("i", len(trees)))
        for t, S in enumerate(trees):
            bk, lk = S.branch_keys(), S.leaf_table()[0]
            f.write(np.array([*S.root_center, S.root_width], np.float32).tobytes() + struct.pack("ii", len(bk), len(lk)) + bk.tobytes() + lk.tobytes())
            f.write(np.array([s["center"][(t, int(key))] for key in lk], np.float32).tobytes())
    r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    _restore(g, s["maps"])
    res, after = _forest(s)
    reg = fl < 0
    assert take(np.float32, n).tobytes() == res.flatness.tobytes()
    assert np.array_equal(take(np.int32, n), np.where(reg, 0, 5))                                 # priorityReduction_ (:399)
    gone = (res.removed != 0) | (res.split != 0)
    assert np.array_equal(take(np.int32, n), np.where(gone, 0, cells.n_images))                   # images_ cleared
    assert np.array_equal(take(np.int32, n), res.n_neighbours) and np.array_equal(take(np.int32, n), res.support)
    assert np.array_equal(take(np.uint8, n), res.removed) and np.array_equal(take(np.uint8, n), res.split)
    assert np.array_equal(take(np.uint8, 4 * n).reshape(n, 4).astype(bool), res.children)
    assert take(np.uint64, 4 * n).tobytes() == res.child_key.tobytes()
    cn = take(np.float32, 32 * n).reshape(4 * n, 8)
    assert cn[:, :4].tobytes() == res.candidates.center.tobytes() and cn[:, 4:].tobytes() == res.candidates.normal.tobytes()
    for t, S in enumerate(after):
        nb, nl = (int(x) for x in take(np.int32, 2))
        bk, lk = take(np.uint64, nb).tolist(), take(np.uint64, nl).tolist()
        pc = take(np.float32, 3 * nl).reshape(nl, 3)
        assert len(set(bk)) == nb and set(bk) == S.branches and len(set(lk)) == nl and set(lk) == set(S.leaves), t
        for key, c in zip(lk, pc):                                       # data[0]'s centre: the seed's, or the first child's
            row = S.leaves[key]
            want = res.candidates.center[row[1], :3] if isinstance(row, tuple) else s["center"][(t, key)]
            assert c.tobytes() == np.asarray(want, np.float32).tobytes(), (t, key)
    v, b, f = api.depth_gates_batch(g, cells, 1.0, 0)
    assert np.array_equal(take(np.int32, n), v) and np.array_equal(take(np.int32, n), b) and np.array_equal(take(np.int32, n), f)
    assert off == len(buf)
    print("cpp process level forest: cells", n, "regularized", int(reg.sum()), "removed", int(res.removed.sum()), "split", int(res.split.sum()))
    assert res.removed.sum() > 0 and res.split.sum() > 0 and reg.sum() > 0
    del frontier
