"""hpmvs_octree_locate_batch on the GPU equals the g++ build of the same header (tests/octree_host.cpp over
hpmvs_amd/csrc/octree.hpp, pinned to the pointer tree by tests/test_cpu_octree_index.py) byte for byte on all six outputs: host
and device pointers; 0, 1, 63, 64, 65 and 20 000 points; the empty tree, one 21-level chain, a random tree of about 5 000 leaves,
and a call without add_width.  Every kind of malformed table is refused with the outputs untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import octree_tree_ref as otr

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = (0, 1, 63, 64, 65, 20000)
HPMVS_ERR_ARG = -2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return otr.HostOctree(tmp_path_factory.mktemp("octree_host"))


def _empty():
    return np.array([1, 2, 3], f32), f32(4.0), np.zeros(0, np.uint64), np.zeros(0, np.uint64)


def _chain():
    """branches at depths 1 .. 20 along one path, one nonempty leaf at depth 21 and one at depth 7 beside the path"""
    rng = np.random.default_rng(21)
    key, branches = 1, []
    for _ in range(20):
        key = (key << 3) | int(rng.integers(8))
        branches.append(key)
    side = (branches[5] << 3) | ((branches[6] & 7) ^ 1)
    return np.array([-0.5, 0.25, 8.0], f32), f32(3.0), np.array(branches, np.uint64), np.array([(key << 3) | 6, side], np.uint64)


@functools.lru_cache(maxsize=None)
def _random():
    rng = np.random.default_rng(5000)
    center, W = np.array([0.5, -1.0, 2.0], f32), f32(7.0)
    T = otr.Tree(center, W)
    pts = (rng.uniform(-0.5, 0.5, (5600, 3)) * float(W) + center).astype(f32)
    for i, p in enumerate(pts):
        T.add_at(p, i, f32(float(W) * 2.0 ** -rng.uniform(3, 11)))
    for i in rng.integers(0, len(pts), 300):                  # empty leaves below branches, collapsed parents
        T.remove(T.at(pts[i]))
    branches, leaves, _ = T.key_sets()
    return center, W, rng.permutation(np.array(sorted(branches), np.uint64)), rng.permutation(np.array(sorted(leaves), np.uint64))


TREES = {"empty": _empty, "chain": _chain, "random": _random, "random-no-add-width": _random}


def _cell_of(center, W, key):
    """(c_, width_) of a path key by Cell(parent, idx)"""
    c, w = np.array(center, f32), f32(W)
    d = (int(key).bit_length() - 1) // 3
    for lvl in range(d):
        idx = (int(key) >> (3 * (d - 1 - lvl))) & 7
        w = f32(float(w) / 2.0)
        c = np.array([float(c[k]) + (1.0 if (idx >> k) & 1 else -1.0) * float(w) / 2.0 for k in range(3)], f32)
    return c, w


def _points(rng, center, W, bk, lk, n):
    """inside, outside, on the split planes of cells of the tree (their centres), the root's faces, NaN / inf"""
    p = (center + rng.uniform(-0.5, 0.5, (n, 3)) * float(W)).astype(f32)
    kind = rng.integers(0, 10, n)
    out = kind == 0
    p[out] = (center + rng.uniform(-1.5, 1.5, (int(out.sum()), 3)) * float(W)).astype(f32)
    keys = np.concatenate([bk, lk])
    if len(keys):
        cells = {}
        for i in np.nonzero(kind == 1)[0]:
            k = int(keys[rng.integers(len(keys))])
            if k not in cells:
                cells[k] = _cell_of(center, W, k)
            c, w = cells[k]
            axes = rng.random(3) < 0.6
            q = (c + rng.uniform(-0.5, 0.5, 3) * float(w)).astype(f32)
            q[axes] = c[axes]
            p[i] = q
    hw = f32(float(W) / 2.0)
    for i in np.nonzero(kind == 2)[0]:
        k = int(rng.integers(3))
        face = f32(center[k] + (hw if rng.random() < 0.5 else -hw))
        p[i, k] = [face, np.nextafter(face, f32(np.inf)), np.nextafter(face, f32(-np.inf))][int(rng.integers(3))]
    odd = np.nonzero(kind == 3)[0][:40]
    for j, i in enumerate(odd):
        p[i, j % 3] = [np.nan, np.inf, -np.inf][(j // 3) % 3]
    return p


def _device_call(scene, center, W, bk, lk, pts, aw, fill=None):
    """the call with device pointers; -> (status, outputs as numpy)"""
    import torch
    from hpmvs_amd import api
    n = len(pts)
    dev = "cuda"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev)
    tb, tl = up(bk, np.int64), up(lk, np.int64)
    tp = up(pts, f32)
    ta = None if aw is None else up(aw, f32)
    outs = []
    for name, dt, shape in otr.OUTPUTS:
        a = np.zeros((n,) + shape, dt)
        if fill is not None:
            a.view(np.uint8)[...] = fill
        outs.append(up(a, np.uint8))
    t = api.OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(center[k])
    t.root_width = float(W)
    t.n_branches, t.n_leaves = len(bk), len(lk)
    t.branch_key, t.leaf_key = tb.data_ptr(), tl.data_ptr()
    rc = api.lib().hpmvs_octree_locate_batch(scene.h, C.byref(t), n, tp.data_ptr(), None if ta is None else ta.data_ptr(),
                                             *[o.data_ptr() for o in outs], 1, None)
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy().tobytes() for o in outs]


@pytest.mark.parametrize("tree", list(TREES))
def test_kernel_equals_the_host_build(gpu_scene, host, tree):
    from hpmvs_amd import api
    center, W, bk, lk = TREES[tree]()
    rng = np.random.default_rng(len(tree))
    seen = dict(nonempty=0, empty=0, outside=0, refused=0, split=0)
    for n in COUNTS:
        pts = _points(rng, center, W, bk, lk, n)
        aw = None if tree.endswith("no-add-width") else (float(W) * 2.0 ** -rng.uniform(0, 12, n)).astype(f32)
        if aw is not None and n:
            aw[::5] = (float(W) * 2.0 ** -rng.integers(1, 12, len(aw[::5]))).astype(f32) * f32(0.9)
        rc, verdict, ref = host.locate(center, W, bk, lk, pts, aw)
        assert rc == 0
        got = api.octree_locate_batch(gpu_scene, center, W, bk, lk, pts.reshape(n, 3), aw)
        for (name, _, _), want in zip(otr.OUTPUTS, ref.bytes()):
            have = getattr(got, name)
            assert have.tobytes() == want, (tree, n, name, np.nonzero(have.reshape(n, -1) != getattr(ref, name).reshape(n, -1))[0][:5])
        rc, dev = _device_call(gpu_scene, center, W, bk, lk, pts, aw)
        assert rc == 0 and dev == ref.bytes(), (tree, n, "device pointers")
        seen["nonempty"] += int((ref.leaf_index >= 0).sum()); seen["empty"] += int((ref.leaf_index < 0).sum())
        seen["outside"] += int((ref.inside == 0).sum())
        seen["refused"] += int(((ref.target_key == 0) & (ref.leaf_index < 0)).sum())
        seen["split"] += int(((ref.target_key != 0) & (ref.target_key != ref.leaf_key)).sum())
    print("octree_locate", tree, "branches", len(bk), "leaves", len(lk), seen)
    assert seen["empty"] > 1000 and seen["outside"] > 500
    if tree == "random":
        assert 4500 <= len(lk) <= 5500 and min(seen.values()) > 500, seen
    if tree.endswith("no-add-width"):
        assert seen["split"] == 0


def test_chain_is_followed_to_depth_21(gpu_scene, host):
    from hpmvs_amd import api
    center, W, bk, lk = _chain()
    deep, side = int(lk[0]), int(lk[1])
    pts = np.array([_cell_of(center, W, deep)[0], _cell_of(center, W, side)[0], _cell_of(center, W, deep ^ 1)[0]], f32)
    aw = np.full(3, 1e-9, f32)
    rc, _, ref = host.locate(center, W, bk, lk, pts, aw)
    got = api.octree_locate_batch(gpu_scene, center, W, bk, lk, pts, aw)
    assert rc == 0 and [getattr(got, n).tobytes() for n, _, _ in otr.OUTPUTS] == ref.bytes()
    assert got.leaf_key.tolist() == [deep, side, deep ^ 1] and got.leaf_index.tolist() == [0, 1, -1]
    assert got.target_key.tolist() == [0, 0, deep ^ 1]        # the empty depth-21 leaf takes it: no level below to split to


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
    ok = api.octree_locate_batch(gpu_scene, center, W, good_b, good_l, pts, aw)
    assert (ok.leaf_index >= 0).any()
    for what, (bk, lk) in cases.items():
        bk, lk = np.array(bk, np.uint64), np.array(lk, np.uint64)
        outs = []
        for name, dt, shape in otr.OUTPUTS:
            a = np.zeros((n,) + shape, dt)
            a.view(np.uint8)[...] = 0x5A
            outs.append(a)
        t = api.OctreeIndex()
        t.root_width = 2.0
        t.n_branches, t.n_leaves = len(bk), len(lk)
        t.branch_key, t.leaf_key = bk.ctypes.data, lk.ctypes.data
        rc = api.lib().hpmvs_octree_locate_batch(gpu_scene.h, C.byref(t), n, pts.ctypes.data, aw.ctypes.data,
                                                 *[o.ctypes.data for o in outs], 0, None)
        assert rc == HPMVS_ERR_ARG and all((o.view(np.uint8) == 0x5A).all() for o in outs), what
        rc, dev = _device_call(gpu_scene, center, W, bk, lk, pts, aw, fill=0x5A)
        assert rc == HPMVS_ERR_ARG and all(set(b) == {0x5A} for b in dev), what
    with pytest.raises(api.HpmvsError):
        api.octree_locate_batch(gpu_scene, [0, np.nan, 0], 2.0, [], [], pts)
    with pytest.raises(api.HpmvsError):
        api.octree_locate_batch(gpu_scene, center, 0.0, [], [], pts)
