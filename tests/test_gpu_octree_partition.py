"""hpmvs_octree_partition on the GPU equals the g++ build of the same header (tests/octree_partition_host.cpp over
hpmvs_amd/csrc/octree.hpp, pinned to the loop of main's getSubTrees on the pointer tree by tests/test_cpu_octree_partition.py) byte
for byte in the info record and every array, with host and device pointers: on the empty tree, the 21-level chain, the random tree
of about 5 000 leaves and the crafted trees, for every min_trees x min_split_leaves of the CPU test, and on trees of 63, 64, 65,
255, 256 and 257 leaves; the calls that must be refused are refused with their outputs untouched; and on the BASELINE
configs[0] scene the subtrees of frontier.partition are Octree.subtree's, route_border finds every leaf's subtree again, and the
sizes and the histogram add up."""
import ctypes as C
import itertools

import numpy as np
import pytest

import octree_partition_ref as opr

pytestmark = pytest.mark.gpu
f32 = np.float32
HPMVS_ERR_ARG = -2
PARAMS = list(itertools.product(opr.MIN_TREES, opr.MIN_SPLIT_LEAVES))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return opr.HostPartition(tmp_path_factory.mktemp("octree_partition_host"))


def _index(center, W, n_branches, n_leaves, branch_ptr, leaf_ptr):
    from hpmvs_amd import api
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(center[k])
    t.root_width = float(W)
    t.n_branches, t.n_leaves = n_branches, n_leaves
    t.branch_key, t.leaf_key = branch_ptr, leaf_ptr
    return t


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def _host_call(scene, center, W, bk, lk, min_trees, min_split, fill=0):
    """the call with host pointers; -> (status, Arrays)"""
    from hpmvs_amd import api
    r = opr.Arrays(len(bk), len(lk), min_trees, fill)
    info = api.OctreePartitionInfo()
    C.memset(C.byref(info), fill, C.sizeof(info))
    t = _index(center, W, len(bk), len(lk), bk.ctypes.data, lk.ctypes.data)
    rc = api.lib().hpmvs_octree_partition(scene.h, C.byref(t), min_trees, min_split, C.byref(info),
                                          *[getattr(r, name).ctypes.data for name, _, _ in opr.OUTPUTS], 0, None)
    r.info[:] = np.frombuffer(bytes(info), np.int32)
    return rc, r


def _device_call(scene, center, W, bk, lk, min_trees, min_split, fill=0):
    """the call with device pointers; -> (status, Arrays)"""
    import torch
    from hpmvs_amd import api
    r = opr.Arrays(len(bk), len(lk), min_trees, fill)
    info = api.OctreePartitionInfo()
    C.memset(C.byref(info), fill, C.sizeof(info))
    tb, tl = _up(bk), _up(lk)
    outs = [_up(getattr(r, name)) for name, _, _ in opr.OUTPUTS]
    t = _index(center, W, len(bk), len(lk), tb.data_ptr(), tl.data_ptr())
    rc = api.lib().hpmvs_octree_partition(scene.h, C.byref(t), min_trees, min_split, C.byref(info), *[o.data_ptr() for o in outs], 1, None)
    torch.cuda.synchronize()
    for (name, dt, _), o in zip(opr.OUTPUTS, outs):
        a = getattr(r, name)
        a[...] = o.cpu().numpy().view(dt).reshape(a.shape)
    r.info[:] = np.frombuffer(bytes(info), np.int32)
    return rc, r


@pytest.mark.parametrize("name", list(opr.TREES) + [str(n) for n in opr.EDGE_LEAVES])
def test_kernels_equal_the_host_build(gpu_scene, host, name):
    center, W, bk, lk = opr.tree(name)
    stops = set()
    for min_trees, min_split in PARAMS:
        rc, want = host.partition(center, W, bk, lk, min_trees, min_split)
        assert rc == 0
        rc, got = _host_call(gpu_scene, center, W, bk, lk, min_trees, min_split)
        assert rc == 0 and not got.differences(want), (name, min_trees, min_split, "host pointers", got.differences(want))
        rc, got = _device_call(gpu_scene, center, W, bk, lk, min_trees, min_split)
        assert rc == 0 and not got.differences(want), (name, min_trees, min_split, "device pointers", got.differences(want))
        stops.add(int(want.info[3]))
    print("octree_partition", name, len(bk), "branches", len(lk), "leaves, stops", sorted(stops))
    assert stops == {0, 1, 2} or (name in ("empty", "chain") and stops == {0, 2})


def test_api_and_nullable_outputs(gpu_scene, host):
    from hpmvs_amd import api
    center, W, bk, lk = opr.tree("random")
    rc, want = host.partition(center, W, bk, lk, 100, 100)
    P = api.octree_partition(gpu_scene, center, W, bk, lk)     # the reference's defaults: 100 subtrees, 100 leaves
    assert [P.n_trees, P.n_orphans, P.n_splits, P.stop] == list(want.info[:4]) and P.histogram.tobytes() == want.info[4:].tobytes()
    assert all(getattr(P, name).tobytes() == getattr(want, name).tobytes() for name, _, _ in opr.OUTPUTS)
    assert P.n_trees > 8 and P.n_splits > 0 and P.stop in (1, 2)
    info = api.OctreePartitionInfo()
    t = _index(center, W, len(bk), len(lk), bk.ctypes.data, lk.ctypes.data)
    rc = api.lib().hpmvs_octree_partition(gpu_scene.h, C.byref(t), 100, 100, C.byref(info), *[None] * 9, 0, None)
    assert rc == 0 and np.frombuffer(bytes(info), np.int32).tobytes() == want.info.tobytes()
    only = opr.Arrays(len(bk), len(lk), 100)
    rc = api.lib().hpmvs_octree_partition(gpu_scene.h, C.byref(t), 100, 100, C.byref(info), *[None] * 5, only.leaf_tree.ctypes.data,
                                          None, None, only.branch_sub_key.ctypes.data, 0, None)
    assert rc == 0 and only.leaf_tree.tobytes() == want.leaf_tree.tobytes() and only.branch_sub_key.tobytes() == want.branch_sub_key.tobytes()


def test_refusals_leave_the_outputs_untouched(gpu_scene):
    center, W = np.zeros(3, f32), f32(2.0)
    good_b, good_l = [0o11, 0o112], [0o1123, 0o12]
    cases = {"a leaf twice": (center, W, good_b, good_l + [0o12], 8, 100), "an orphan key": (center, W, good_b, good_l + [0o1333], 8, 100),
             "min_trees = 4097": (center, W, good_b, good_l, 4097, 100), "min_split_leaves = 0": (center, W, good_b, good_l, 8, 0),
             "a root without width": (center, f32(0.0), good_b, good_l, 8, 100),
             "a root that is not finite": (np.array([0, np.nan, 0], f32), W, good_b, good_l, 8, 100)}
    rc, ok = _host_call(gpu_scene, center, W, np.array(good_b, np.uint64), np.array(good_l, np.uint64), 8, 100)
    assert rc == 0 and ok.info[0] == 1 and ok.root_key[0] == 0o11
    for what, (c, w, bk, lk, min_trees, min_split) in cases.items():
        bk, lk = np.array(bk, np.uint64), np.array(lk, np.uint64)
        for call in (_host_call, _device_call):
            rc, r = call(gpu_scene, c, w, bk, lk, min_trees, min_split, fill=0x5A)
            assert rc == HPMVS_ERR_ARG and all(set(b) <= {0x5A} for b in r.bytes()), (what, call.__name__)


def test_seed_tree_of_a_scene_partitions_into_its_subtrees(tiny_scene, gpu_scene):
    from hpmvs_amd import api, frontier, synth
    xyz, off, img = synth.make_nvm_points(tiny_scene, 400, start_level=2, noise=1.0)
    batch = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, max_images=64)
    T = frontier.seed_tree(gpu_scene, batch, patch_init_maxlevel=9, set_depths=False)
    O = frontier.Octree.from_seed_tree(T)
    P = frontier.partition(gpu_scene, O, min_trees=8, min_split_leaves=3)
    A = P.arrays
    assert len(P.trees) == A.n_trees >= 2 and len(O.leaves) > 50
    for t, sub in enumerate(P.trees):
        want = O.subtree(int(P.root_key[t]))
        assert sub.branches == want.branches and sub.leaves == want.leaves and sub.root_level == want.root_level
        assert sub.root_center.tobytes() == want.root_center.tobytes() and sub.root_width.tobytes() == want.root_width.tobytes()
        assert [k for _, k in P.queues[t]] == [int(k) for k in want.leaf_table()[0]]
    lk, _, cc, _ = O.leaf_table()
    held = A.leaf_tree >= 0
    assert frontier.route_border(gpu_scene, P.trees, cc[held]).tobytes() == A.leaf_tree[held].tobytes()
    n = A.n_trees
    assert A.tree_leaves[:n].sum() + A.n_orphans == len(lk) == P.histogram.sum() and len(P.orphans) == A.n_orphans
    print("octree_partition scene:", len(lk), "leaves,", n, "subtrees,", A.n_orphans, "orphans, stop", P.stop, "histogram", P.histogram.tolist())
