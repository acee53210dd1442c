"""hpmvs_border_forest_batch against the g++ build of octree.hpp's border_forest_sequential (tests/border_forest_host.cpp, pinned
by tests/test_cpu_border_forest.py to ot_route and per-tree ot_insert): every byte of tree, accepted, leaf_key and blocker, with host
pointers and with device pointers, on poisoned outputs.

  forests       the CPU test's: the special forest (a keyless tree, a one-key tree, identical key sets under two roots, a shared
                face, nested roots) with its queue of 3 000, runs of 150 and 70 members on the same sub-key of two trees
                interleaved in the queue, four trees of four root widths, 130 trees, one tree, no tree; n = 0, 1, 65
  nullable      blocker absent; no result at all
  refusals      a bad key in a middle tree, bad offsets: the lowest tree is named, the outputs stay poisoned and every depth-map
                cell stays as it was; set_depths on a scene without maps is HPMVS_ERR_STATE
  depths        after the call the maps equal those of a twin scene that ran route_border and insert_border per destination
                tree, on refined seeds delivered into the subtrees of a seed tree built from the other half of the seeds"""
import ctypes as C

import numpy as np
import pytest

import border_forest_ref as bfr

pytestmark = pytest.mark.gpu
f32 = np.float32
HPMVS_ERR_ARG, HPMVS_ERR_STATE = -2, -3
NAMES = ("tree", "accepted", "leaf_key", "blocker")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bfr.HostBorder(tmp_path_factory.mktemp("border_forest_host"))


@pytest.fixture(scope="module")
def world():
    """the GPU scene with depth maps, its twin, one without maps, and refined seeds: the even rows built into a seed tree whose
    depth-1 subtrees are the forest, the odd rows the border queue"""
    from hpmvs_amd import api, frontier, synth
    scene = synth.make_scene(3, 640, 480, n_waves=24)
    g, twin, bare = api.Scene(scene, device=0), api.Scene(scene, device=0), api.Scene(scene, device=0)
    b = api.Batch.from_seeds(synth.make_seeds(scene, 600, start_level=2))
    api.optimize_batch(g, b)
    k = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
    R.ok[:] = 1
    even, border = frontier._rows(R, np.arange(0, R.n, 2)), frontier._rows(R, np.arange(1, R.n, 2))
    even.ok[:] = 1
    border.scale[::2] *= f32(0.5)                               # (every second one at half its scale: narrow leaves take some too)
    T = frontier.seed_tree(g, even, patch_init_maxlevel=9, set_depths=False)
    yield dict(g=g, twin=twin, bare=bare, T=T, border=border)
    for s in (g, twin, bare):
        s.close()


def _subtrees(T):
    from hpmvs_amd import frontier
    O = frontier.Octree.from_seed_tree(T)
    return [O.subtree(k) for k in sorted(k for k in O.branches if frontier.key_depth(k) == 1)]


def _maps(g):
    from hpmvs_amd import api
    return [api.depth_level(g, v, l).copy() for v in range(g.n_views) for l in range(g.view_levels[v])]


def _batch(center, scale):
    """a patch batch around the centres and scales of a synthetic queue: no images (nothing for set_depths to write)"""
    from hpmvs_amd import api
    n = len(scale)
    return api.Batch(center, np.zeros((n, 4), f32), scale, np.zeros(n, np.int32), np.full((n, 4), -1, np.int32))


def call(g, device, trees, batch, set_depths=0, null=(), no_result=False, bf=None, lf=None):
    """one hpmvs_border_forest_batch through api.lib() on poisoned outputs -> (status, Delivered, message)"""
    from hpmvs_amd import api
    roots, bf0, lf0, bk, lk = bfr.flatten(trees)
    bfirst = bf0 if bf is None else np.asarray(bf, np.int32)
    lfirst = lf0 if lf is None else np.asarray(lf, np.int32)
    out = bfr.Delivered(batch.n, poison=True)
    keep, dev = [], {}
    if device:
        import torch
        up = lambda a: (keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")) or keep[-1].data_ptr()) if a.size else None
        pb = api.PatchBatch()
        pb.n, pb.max_images = batch.n, batch.max_images
        for name in ("center", "normal", "scale", "n_images", "images"):
            setattr(pb, name, up(getattr(batch, name)))
        pbk, plk = up(bk), up(lk)
        for name in NAMES:
            dev[name] = torch.from_numpy(getattr(out, name).view(np.uint8).reshape(-1).copy()).to("cuda:0")
        ptr = lambda name: dev[name].data_ptr() if batch.n else None
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device="cuda:0")
        sp = C.c_void_p(stream.cuda_stream)
    else:
        pb = batch.c_struct()
        pb.ok = None                                            # neither read nor written
        pbk, plk, sp = bk.ctypes.data, lk.ctypes.data, None
        ptr = lambda name: getattr(out, name).ctypes.data
    f = api.OctreeForest()
    f.n_trees = len(trees)
    f.root, f.branch_first, f.leaf_first, f.branch_key, f.leaf_key = roots.ctypes.data, bfirst.ctypes.data, lfirst.ctypes.data, pbk, plk
    res = api.BorderForestResultStruct()
    for name in NAMES:
        setattr(res, name, None if name in null else ptr(name))
    status = api.lib().hpmvs_border_forest_batch(g.h, C.byref(f), C.byref(pb), set_depths, None if no_result else C.byref(res),
                                                 1 if device else 0, sp)
    message = api.lib().hpmvs_last_error().decode()
    if device:
        import torch
        torch.cuda.synchronize()                                # (the call is host-synchronous: nothing of it is left to wait for)
        for name in NAMES:
            a = getattr(out, name)
            a[...] = dev[name].cpu().numpy().view(a.dtype)
    return status, out, message


_cases = {}


def cases(host):
    """name -> (trees, center, scale, the host build's outputs): computed once, shared by both pointer forms"""
    if _cases:
        return _cases
    rng = np.random.default_rng(1750)
    special, center, scale = bfr.special_case()
    made = {"special 3000": (special, center, scale),
            "150 and 70 on one sub-key": (special,) + bfr.crowd(rng, special, [(1, 150), (2, 70)]),
            "four root widths": (bfr.four_widths_forest(),) + bfr.queue(rng, bfr.four_widths_forest(), 1200),
            "130 trees": (bfr.many_trees_forest(130),) + bfr.queue(rng, bfr.many_trees_forest(130), 1500),
            "one tree": (special[:1],) + bfr.queue(rng, special[:1], 500),
            "no tree": ([],) + bfr.queue(rng, [], 70),
            "n = 0": (special, np.zeros((0, 4), f32), np.zeros(0, f32)),
            "n = 0, no tree": ([], np.zeros((0, 4), f32), np.zeros(0, f32))}
    for n in (1, 65):
        made[f"n = {n}"] = (special, center[:n].copy(), scale[:n].copy())
    made["n = 65 in one run"] = (special,) + bfr.crowd(rng, special, [(1, 65)], n_other=0)
    for name, (trees, c, s) in made.items():
        rc, want, found = host.border(trees, c, s)
        assert rc == 0, (name, found)
        _cases[name] = (trees, c, s, want)
    return _cases


@pytest.mark.parametrize("device", (0, 1), ids=("host pointers", "device pointers"))
def test_the_call_equals_the_host_build(host, world, device):
    for name, (trees, center, scale, want) in cases(host).items():
        status, got, message = call(world["g"], device, trees, _batch(center, scale))
        assert status == 0, (name, message)
        for field, a, b in zip(NAMES, got.bytes(), want.bytes()):
            assert a == b, (name, field, np.nonzero(getattr(got, field) != getattr(want, field))[0][:5])
    trees, center, scale, want = _cases["150 and 70 on one sub-key"]
    _, runs = bfr.classes(trees, center, scale, want)
    assert len(runs[(1, 0o17)]) >= 150 and len(runs[(2, 0o17)]) >= 70 and want.accepted[runs[(2, 0o17)]].sum() >= 20
    assert (_cases["no tree"][3].tree == -1).all() and len(set(_cases["130 trees"][3].tree.tolist())) > 120


@pytest.mark.parametrize("device", (0, 1), ids=("host pointers", "device pointers"))
def test_nullable_outputs(host, world, device):
    trees, center, scale, want = cases(host)["special 3000"]
    poison = bfr.Delivered(len(scale), poison=True)
    status, got, message = call(world["g"], device, trees, _batch(center, scale), null=("blocker",))
    assert status == 0, message
    assert got.bytes()[:3] == want.bytes()[:3] and got.blocker.tobytes() == poison.blocker.tobytes()
    for name in ("tree", "accepted", "leaf_key"):
        status, got, message = call(world["g"], device, trees, _batch(center, scale), null=(name,))
        assert status == 0, (name, message)
        for field in NAMES:
            assert getattr(got, field).tobytes() == getattr(poison if field == name else want, field).tobytes(), (name, field)
    status, got, message = call(world["g"], device, trees, _batch(center, scale), no_result=True)
    assert status == 0 and got.bytes() == poison.bytes(), message


def test_depths_equal_route_and_insert_per_tree(world):
    from hpmvs_amd import api, frontier
    g, twin, border = world["g"], world["twin"], world["border"]
    # the twin: today's path
    api.depth_reset(twin)
    subs = _subtrees(world["T"])
    tree = frontier.route_border(twin, subs, border.center)
    accepted = np.zeros(border.n, np.uint8)
    for k in sorted(set(tree.tolist()) - {-1}):
        rows = np.nonzero(tree == k)[0]
        res = frontier.insert_border(twin, subs[k], frontier._rows(border, rows), 0.0)
        accepted[rows[res.accepted]] = 1
    want = _maps(twin)
    assert accepted.sum() >= 20 and len(set(tree[accepted != 0].tolist())) >= 2
    # the one call, with the result and without one
    flat = frontier._flatten_forest(_subtrees(world["T"]))
    for no_result in (False, True):
        api.depth_reset(g)
        before = _maps(g)
        if no_result:
            f, hold = api.octree_forest(*flat)
            bb = border.c_struct()
            api._chk(api.lib().hpmvs_border_forest_batch(g.h, C.byref(f), C.byref(bb), 1, None, 0, None))
        else:
            r = api.border_forest_batch(g, border, *flat, set_depths=True)
            assert r.tree.tobytes() == tree.tobytes() and r.accepted.tobytes() == accepted.tobytes()
        got = _maps(g)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), no_result
        assert sum(int((a != b).sum()) for a, b in zip(got, before)) >= 20
    # set_depths = 0 leaves the maps alone
    api.depth_reset(g)
    before = _maps(g)
    r = api.border_forest_batch(g, border, *flat, set_depths=False)
    assert r.accepted.tobytes() == accepted.tobytes() and all(np.array_equal(a, b) for a, b in zip(_maps(g), before))


@pytest.mark.parametrize("device", (0, 1), ids=("host pointers", "device pointers"))
def test_a_malformed_forest_is_refused_before_any_write(world, device):
    from hpmvs_amd import api, frontier
    g, border = world["g"], world["border"]
    subs = _subtrees(world["T"])
    trees = [(np.array([*S.root_center, S.root_width], f32), S.branch_keys(), S.leaf_table()[0]) for S in subs]
    full = [k for k, t in enumerate(trees) if len(t[2]) >= 2]
    assert len(full) >= 3
    mid, low = full[1], full[0]
    api.depth_reset(g)
    before = _maps(g)
    poison = bfr.Delivered(border.n, poison=True).bytes()
    spoil = {"no path key": lambda bk, lk: (bk, np.append(lk, np.uint64(2))), "twice": lambda bk, lk: (bk, np.append(lk, lk[0])),
             "neither a branch nor the root": lambda bk, lk: (bk, np.append(lk, np.uint64((int(max(lk)) << 6) | 0o11)))}
    for what, fn in spoil.items():
        for which, named in (((mid,), mid), ((full[2], low), low)):
            bad = list(trees)
            for k in which:
                bad[k] = (trees[k][0],) + tuple(np.ascontiguousarray(a, np.uint64) for a in fn(trees[k][1], trees[k][2]))
            status, got, message = call(g, device, bad, border, set_depths=1)
            assert status == HPMVS_ERR_ARG and f"tree {named}:" in message and what in message, (what, message)
            assert got.bytes() == poison
    _, bf, lf, _, _ = bfr.flatten(trees)
    for which in ("bf", "lf"):
        off = (bf if which == "bf" else lf).copy()
        off[mid + 1] = off[mid] - 1
        status, got, message = call(g, device, trees, border, set_depths=1, **{which: off})
        assert status == HPMVS_ERR_ARG and f"tree {mid}:" in message and got.bytes() == poison, message
    root = list(trees)
    root[mid] = (np.array([0, 0, 0, -1], f32),) + trees[mid][1:]
    status, got, message = call(g, device, root, border, set_depths=1)
    assert status == HPMVS_ERR_ARG and f"tree {mid}:" in message and got.bytes() == poison, message
    # a bad batch
    wide = api.Batch(border.center, border.normal, border.scale, border.n_images, border.images)
    wide.max_images = 0
    status, got, message = call(g, device, trees, wide, set_depths=1)
    assert status == HPMVS_ERR_ARG and got.bytes() == poison, message
    assert all(np.array_equal(a, b) for a, b in zip(_maps(g), before))


def test_set_depths_without_maps_is_a_state_error(world):
    from hpmvs_amd import frontier
    border = world["border"]
    subs = _subtrees(world["T"])
    trees = [(np.array([*S.root_center, S.root_width], f32), S.branch_keys(), S.leaf_table()[0]) for S in subs]
    poison = bfr.Delivered(border.n, poison=True).bytes()
    status, got, message = call(world["bare"], 0, trees, border, set_depths=1)
    assert status == HPMVS_ERR_STATE and "hpmvs_scene_depth_reset" in message and got.bytes() == poison, message
    status, got, message = call(world["bare"], 0, trees, border, set_depths=0)
    assert status == 0 and got.accepted.sum() >= 20, message
