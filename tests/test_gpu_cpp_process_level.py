"""The C++ host layer's PatchOptimizer::regularizeLevel / settleLevel / processLevel (tests/native/process_level_cpp.cpp, built here
with g++ against libhpmvs_host.so) and hpmvs_amd.frontier's regularize_level / process_level on the same dumped state: flatness,
neighbour counts, the settle decisions, the sweep's versioned leaf table and the depth maps behind the gates are byte-identical, and
regularizeLevel resets priorityReduction_ as processCell does (CellProcessor.cpp:399)."""
import os
import subprocess

import numpy as np
import pytest

import octree_ref as ot
from test_gpu_cpp_interface import _dump_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state(scene, gscene, rng, n_seeds):
    from hpmvs_amd import api, frontier, synth
    seeds = synth.make_seeds(scene, n_seeds, start_level=2, seed=synth.SEED + 91)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gscene, b)
    keep = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[keep], b.normal[keep], b.scale[keep], b.n_images[keep], b.images[keep])
    P = R.center[:, :3].astype(np.float32)
    lo, hi = P.min(axis=0), P.max(axis=0)
    rc = ((lo + hi) / 2).astype(np.float32)
    rw = np.float32(2.0 ** np.ceil(np.log2(float((hi - lo).max()) * 1.1)))
    width = (R.scale * np.float32(2.0 / 0.9) * np.exp2(rng.integers(0, 2, size=R.n))).astype(np.float32)
    tree = ot.OctTree(rc, rw, P)
    for e in rng.permutation(R.n):
        tree.add(int(e), width[e])
    leaves = tree.nonempty()
    idx = np.array([l.data[0] for l in leaves])[rng.permutation(len(leaves))]
    cells = api.Batch(R.center[idx], R.normal[idx], R.scale[idx], R.n_images[idx], R.images[idx])
    by_patch = {l.data[0]: l for l in leaves}
    cl = [by_patch[i] for i in idx]
    snap = frontier.OctreeSnapshot(rc, rw, np.array([l.c for l in cl]), np.array([l.w for l in cl]), P[idx])
    n = cells.n
    fl = np.where(rng.random(n) < 0.5, -1.0, 0.0).astype(np.float32)
    rem = rng.random(n) < 0.1
    fl[rem] = np.where(rng.random(int(rem.sum())) < 0.5, 2.5, 2.6).astype(np.float32)
    final = (rng.random(n) < 0.3).astype(np.uint8)
    return cells, snap, fl, final


def test_cpp_levels_equal_python(tiny_scene, gpu_scene, tmp_path):
    from hpmvs_amd import api, frontier
    exe = str(tmp_path / "process_level_cpp")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "hpmvs_amd")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + inc, os.path.join(ROOT, "tests", "native", "process_level_cpp.cpp"), "-o", exe,
                    "-L" + lib, "-lhpmvs_host", "-lhpmvs_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
    rng = np.random.default_rng(17)
    cells, snap, fl0, final = _state(tiny_scene, gpu_scene, rng, 700)
    n = cells.n
    dump, outp = tmp_path / "state.bin", tmp_path / "out.bin"
    _dump_scene(dump, tiny_scene, cells, n)
    with open(dump, "ab") as f:
        for i in range(n):
            f.write(np.float32(fl0[i]).tobytes() + np.int32(i).tobytes() + np.uint8(final[i]).tobytes())
        f.write(snap.root_center.astype(np.float32).tobytes() + np.float32(snap.root_width).tobytes() + np.int32(snap.n).tobytes())
        f.write(snap.cell_center.tobytes() + snap.cell_width.tobytes() + snap.patch_center.tobytes())
    r = subprocess.run([exe, str(dump), str(outp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a

    # (A) regularizeLevel == regularize_level (every cell, flatness -1, position = index, the sweep-start table)
    fl_a, nn_a, reset = take(np.float32, n), take(np.int32, n), int(take(np.int32, 1)[0])
    cw = snap.cell_width.copy()
    f_py, n_py, _ = frontier.regularize_level(gpu_scene, cells, cw, np.arange(n), np.ones(n, np.uint8), snap, np.full(n, -1.0, np.float32))
    assert fl_a.tobytes() == f_py.tobytes() and np.array_equal(nn_a, n_py)
    assert reset == n
    # (B) processLevel == process_level on the same maps
    api.depth_reset(gpu_scene)
    cells.ok[:] = 1
    api.set_depths_batch(gpu_scene, cells)
    res = frontier.process_level(gpu_scene, cells, np.arange(n), fl0, np.ones(n, np.uint8), snap, final)
    fl_b, nn_b = take(np.float32, n), take(np.int32, n)
    assert fl_b.tobytes() == res.flatness.tobytes() and np.array_equal(nn_b, res.n_neighbours)
    S = int(take(np.int32, 1)[0])
    assert S == len(res.settled)
    rec = np.dtype([("i", "<i4"), ("rem", "u1"), ("split", "u1"), ("sup", "<i4"), ("child", "u1", 4), ("oct", "<i4", 4), ("leaf", "<i4", 4)])
    rows = take(rec, S)
    st = res.settle
    assert np.array_equal(rows["i"], res.settled)
    assert np.array_equal(rows["rem"], st.removed) and np.array_equal(rows["split"], st.split) and np.array_equal(rows["sup"], st.support)
    assert np.array_equal(rows["child"].astype(bool), st.children) and np.array_equal(rows["oct"], st.child_octant)
    assert np.array_equal(rows["leaf"], res.child_leaf)
    L2 = int(take(np.int32, 1)[0])
    t = res.snapshot
    assert L2 == t.n
    assert take(np.float32, 3 * L2).tobytes() == t.cell_center.tobytes() and take(np.float32, L2).tobytes() == t.cell_width.tobytes()
    assert take(np.float32, 3 * L2).tobytes() == t.patch_center.tobytes()
    assert np.array_equal(take(np.int32, L2), t.born) and np.array_equal(take(np.int32, L2), t.died)
    v, b, f = api.depth_gates_batch(gpu_scene, cells, 1.0, 0)
    assert np.array_equal(take(np.int32, n), v) and np.array_equal(take(np.int32, n), b) and np.array_equal(take(np.int32, n), f)
    assert off == len(buf)
    print("cpp process level: cells", n, "settled", S, "removed", int(st.removed.sum()), "split", int(st.split.sum()), "leaves", L2)
    assert st.removed.sum() > 0 and st.split.sum() > 0 and L2 > snap.n and (res.n_neighbours >= 4).sum() > 0
