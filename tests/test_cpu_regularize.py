"""Host side of the regularize path that needs no device: the C entry refuses to run without a GPU, and the scheduler-side
octree helpers of hpmvs_amd.frontier (Cell(parent, idx), Branch::at's octant) agree with the DynOctTree restatement."""
import ctypes as C

import numpy as np

import octree_ref as ot


def test_regularize_batch_has_no_cpu_fallback():
    from hpmvs_amd import api
    if api.device_count() > 0:
        return  # on a GPU box tests/test_gpu_regularize_level.py covers the call
    b = api.Batch(np.zeros((1, 4)), np.zeros((1, 4)), np.zeros(1), np.ones(1), np.zeros((1, 1)))
    t = api.LeafTable()
    rc = api.lib().hpmvs_regularize_batch(None, C.byref(b.c_struct()), None, None, None, C.byref(t), None, None, None, 0, None)
    assert rc == -4  # HPMVS_ERR_NODEVICE


def test_child_cells_and_octants_follow_the_tree():
    from hpmvs_amd import frontier
    rng = np.random.default_rng(1)
    P = (rng.random((400, 3)) * 7.3 - 2.1).astype(np.float32)
    t = ot.OctTree(np.float32([1.55, 1.55, 1.55]), np.float32(8.0), P)
    for e in range(len(P)):
        t.add(e, np.float32(0.1 * 2 ** rng.integers(0, 4)))
    leaves = t.nonempty()
    assert len({t.depth(l) for l in leaves}) >= 3
    for l in leaves:
        par = l.parent
        idx = frontier.octant(par.c, l.c)
        c, w = frontier.child_cell(par.c, par.w, idx)
        assert c.tobytes() == np.asarray(l.c, np.float32).tobytes() and w == l.w
        assert t.at(P[l.data[0]]) is l
