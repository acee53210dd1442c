"""hpmvs_octree_insert_batch and hpmvs_octree_route_batch on the GPU equal the g++ build of the same header
(tests/octree_insert_host.cpp over hpmvs_amd/csrc/octree.hpp, pinned to the pointer tree by tests/test_cpu_octree_insert.py) byte
for byte on every output, with host and device pointers: 0, 1, 63, 64, 65 and 6 000 patches on the empty tree, the 21-level
chain and a random tree of about 5 000 leaves; every patch in a static leaf of its own, one run of 4 000 members (an accepted
list of many strides of 64) and many runs of 1 .. 70 members; a call without `blocker`; every kind of malformed table refused
with the outputs untouched; routing over 0, 1 and 130 roots."""
import ctypes as C

import numpy as np
import pytest

import octree_insert_ref as oir

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = (0, 1, 63, 64, 65, 6000)
HPMVS_ERR_ARG = -2
OUTPUTS = (("accepted", np.uint8), ("leaf_key", np.uint64), ("blocker", np.int32))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return oir.HostInsert(tmp_path_factory.mktemp("octree_insert_host"))


def _index(center, W, n_branches, n_leaves, branch_ptr, leaf_ptr):
    from hpmvs_amd import api
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(center[k])
    t.root_width = float(W)
    t.n_branches, t.n_leaves = n_branches, n_leaves
    t.branch_key, t.leaf_key = branch_ptr, leaf_ptr
    return t


def _up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to("cuda")


def _device_call(scene, center, W, bk, lk, pts, aw, fill=None, blocker=True):
    """the call with device pointers; -> (status, outputs as bytes)"""
    import torch
    from hpmvs_amd import api
    n = len(pts)
    tb, tl, tp, ta = _up(bk, np.int64), _up(lk, np.int64), _up(pts, f32), _up(aw, f32)
    outs = []
    for _, dt in OUTPUTS:
        a = np.zeros(n, dt)
        if fill is not None:
            a.view(np.uint8)[...] = fill
        outs.append(_up(a, np.uint8))
    t = _index(center, W, len(bk), len(lk), tb.data_ptr(), tl.data_ptr())
    rc = api.lib().hpmvs_octree_insert_batch(scene.h, C.byref(t), n, tp.data_ptr(), ta.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                             outs[2].data_ptr() if blocker else None, 1, None)
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy().tobytes() for o in outs]


def _check(scene, host, tree, pts, aw, what):
    """host and device pointers against the g++ build; -> its result"""
    from hpmvs_amd import api
    center, W, bk, lk = tree
    rc, ref = host.insert(center, W, bk, lk, pts, aw)
    assert rc == 0
    got = api.octree_insert_batch(scene, center, W, bk, lk, pts.reshape(len(pts), 3), aw)
    for name, _ in OUTPUTS:
        have, want = getattr(got, name), getattr(ref, name)
        assert have.tobytes() == want.tobytes(), (what, name, np.nonzero(have != want)[0][:5])
    rc, dev = _device_call(scene, center, W, bk, lk, pts, aw)
    assert rc == 0 and dev == ref.bytes(), (what, "device pointers")
    return ref


@pytest.mark.parametrize("name", list(oir.TREES))
def test_kernels_equal_the_host_build(gpu_scene, host, name):
    seen = dict(accepted=0, refused_by_tree=0, refused_by_earlier=0)
    for n in COUNTS:
        tree, pts, aw = oir.case(name, n)
        ref = _check(gpu_scene, host, tree, pts, aw, (name, n))
        seen["accepted"] += int(ref.accepted.sum())
        seen["refused_by_tree"] += int(((ref.accepted == 0) & (ref.blocker < 0)).sum())
        seen["refused_by_earlier"] += int((ref.blocker >= 0).sum())
    print("octree_insert", name, seen)
    assert min(seen.values()) > 200, seen


def _empty_leaves(center, W, bk, lk):
    """keys of the empty leaves of a tree: children of a branch (or of the root) that are in neither set"""
    have = {int(k) for k in bk} | {int(k) for k in lk}
    return [(b << 3) | i for b in [1] + sorted(int(k) for k in bk) for i in range(8) if ((b << 3) | i) not in have]


def _inside(rng, center, W, key, g):
    """g points well inside the cell `key`"""
    c, w = oir.cell_of(center, W, key)
    return (c + rng.uniform(-0.45, 0.45, (g, 3)) * float(w)).astype(f32), np.full(g, w, f32)


def test_every_patch_in_a_leaf_of_its_own(gpu_scene, host):
    rng = np.random.default_rng(1)
    tree = oir.random_tree()
    cells = _empty_leaves(*tree)
    cells = [cells[i] for i in rng.permutation(len(cells))[:3000]]
    got = [_inside(rng, tree[0], tree[1], k, 1) for k in cells]
    pts, w = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    aw = (w * 2.0 ** rng.uniform(-3, 0, len(w))).astype(f32)
    ref = _check(gpu_scene, host, tree, pts, aw, "own leaf")
    assert len(pts) == 3000 and ref.accepted.all() and (ref.blocker == -1).all()
    assert len(set(int(k) >> (3 * (oir.key_depth(k) - oir.key_depth(c))) for k, c in zip(ref.leaf_key, cells))) == 3000


def test_one_run_of_4000_members(gpu_scene, host):
    rng = np.random.default_rng(4000)
    tree = oir.empty_tree()                                    # octant 7 of the empty tree: ONE empty leaf of depth 1
    center, W = tree[0], tree[1]
    pts = (center + rng.uniform(0.001, 0.499, (4000, 3)) * float(W)).astype(f32)
    pts[::5] = (center + (0.25 + rng.uniform(-0.004, 0.004, (800, 3))) * float(W)).astype(f32)   # long shared prefixes
    aw = (float(W) / 2.0 * 2.0 ** -rng.uniform(2, 10, 4000)).astype(f32)   # small against the leaf: the accepted list grows long
    ref = _check(gpu_scene, host, tree, pts, aw, "one run")
    survivors = (ref.accepted != 0) | (ref.blocker >= 0)
    print("octree_insert one run:", int(survivors.sum()), "members,", int(ref.accepted.sum()), "accepted")
    assert survivors.all() and ref.accepted.sum() > 10 * 64 and (ref.blocker >= 0).sum() > 500


def test_many_runs_of_1_to_70_members(gpu_scene, host):
    rng = np.random.default_rng(70)
    tree = oir.random_tree()
    cells = [k for k in _empty_leaves(*tree) if oir.key_depth(k) <= 6]
    cells = [cells[i] for i in rng.permutation(len(cells))[:140]]
    sizes = [1 + (j % 70) for j in range(len(cells))]
    sizes[:6] = [63, 64, 65, 64, 1, 70]
    got = [_inside(rng, tree[0], tree[1], k, g) for k, g in zip(cells, sizes)]
    pts, w = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    aw = (w * 2.0 ** rng.uniform(-5, 0, len(w))).astype(f32)   # never wider than the static leaf: every patch is a member
    order = rng.permutation(len(pts))                          # the runs interleave in the queue
    pts, aw = pts[order], aw[order]
    ref = _check(gpu_scene, host, tree, pts, aw, "many runs")
    assert len(cells) == 140 and ((ref.accepted != 0) | (ref.blocker >= 0)).all()
    assert ref.accepted.sum() > 1000 and (ref.blocker >= 0).sum() > 500


def test_without_blocker(gpu_scene, host):
    from hpmvs_amd import api
    tree, pts, aw = oir.case("chain", 6000)
    center, W, bk, lk = tree
    rc, ref = host.insert(center, W, bk, lk, pts, aw, blocker=False)
    assert rc == 0
    acc, key = np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.uint64)
    t = _index(center, W, len(bk), len(lk), bk.ctypes.data, lk.ctypes.data)
    rc = api.lib().hpmvs_octree_insert_batch(gpu_scene.h, C.byref(t), len(pts), pts.ctypes.data, aw.ctypes.data, acc.ctypes.data,
                                             key.ctypes.data, None, 0, None)
    assert rc == 0 and [acc.tobytes(), key.tobytes()] == ref.bytes()[:2]
    rc, dev = _device_call(gpu_scene, center, W, bk, lk, pts, aw, fill=0x5A, blocker=False)
    assert rc == 0 and dev[:2] == ref.bytes()[:2] and set(dev[2]) == {0x5A}


def test_malformed_tables_are_refused_with_outputs_untouched(gpu_scene):
    from hpmvs_amd import api
    center, W = np.zeros(3, f32), f32(2.0)
    deep21 = (1 << 63) | 5
    good_b, good_l = [0o11, 0o112], [0o1123, 0o12]
    cases = {
        "orphan leaf": (good_b, good_l + [0o1333]), "orphan branch": (good_b + [0o1455], good_l),
        "branch and leaf": (good_b, good_l + [0o112]), "duplicate leaf": (good_b, good_l + [0o12]),
        "duplicate branch": (good_b + [0o11], good_l), "zero": (good_b, good_l + [0]), "the root": (good_b + [1], good_l),
        "off-grid sentinel": (good_b, good_l + [0o21]), "branch at depth 21": (good_b + [deep21], good_l),
    }
    n = 65
    pts = np.random.default_rng(1).uniform(-1, 1, (n, 3)).astype(f32)
    aw = np.full(n, 0.1, f32)
    ok = api.octree_insert_batch(gpu_scene, center, W, good_b, good_l, pts, aw)
    assert ok.accepted.any() and not ok.accepted.all()
    for what, (bk, lk) in cases.items():
        bk, lk = np.array(bk, np.uint64), np.array(lk, np.uint64)
        outs = []
        for _, dt in OUTPUTS:
            a = np.zeros(n, dt)
            a.view(np.uint8)[...] = 0x5A
            outs.append(a)
        t = _index(center, W, len(bk), len(lk), bk.ctypes.data, lk.ctypes.data)
        rc = api.lib().hpmvs_octree_insert_batch(gpu_scene.h, C.byref(t), n, pts.ctypes.data, aw.ctypes.data,
                                                 *[o.ctypes.data for o in outs], 0, None)
        assert rc == HPMVS_ERR_ARG and all((o.view(np.uint8) == 0x5A).all() for o in outs), what
        rc, dev = _device_call(gpu_scene, center, W, bk, lk, pts, aw, fill=0x5A)
        assert rc == HPMVS_ERR_ARG and all(set(b) == {0x5A} for b in dev), what
    with pytest.raises(api.HpmvsError):
        api.octree_insert_batch(gpu_scene, [0, np.nan, 0], 2.0, [], [], pts, aw)
    with pytest.raises(api.HpmvsError):
        api.octree_insert_batch(gpu_scene, center, 0.0, [], [], pts, aw)


@pytest.mark.parametrize("n_trees", (0, 1, 130))
def test_route_equals_the_host_build(gpu_scene, host, n_trees):
    import torch
    from hpmvs_amd import api
    rng = np.random.default_rng(n_trees)
    for n in COUNTS:
        roots, pts = oir.route_case(rng, n_trees, n)
        want = host.route(roots, pts)
        got = api.octree_route_batch(gpu_scene, roots, pts)
        assert got.tobytes() == want.tobytes(), (n_trees, n, np.nonzero(got != want)[0][:5])
        tp, tt = _up(pts, f32), _up(np.full(n, 0x5A5A5A5A, np.int32), np.int32)
        rc = api.lib().hpmvs_octree_route_batch(gpu_scene.h, n_trees, roots.ctypes.data, n, tp.data_ptr(), tt.data_ptr(), 1, None)
        torch.cuda.synchronize()
        assert rc == 0 and tt.cpu().numpy().tobytes() == want.tobytes(), (n_trees, n, "device pointers")
        if n == 6000 and n_trees == 130:
            assert (want < 0).sum() > 500 and len(set(want.tolist())) > 40
    bad = np.array([[0, 0, 0, 1], [0, np.inf, 0, 1]], f32)
    with pytest.raises(api.HpmvsError):
        api.octree_route_batch(gpu_scene, bad, np.zeros((3, 3), f32))
    bad[1] = [0, 0, 0, 0]
    with pytest.raises(api.HpmvsError):
        api.octree_route_batch(gpu_scene, bad, np.zeros((3, 3), f32))
