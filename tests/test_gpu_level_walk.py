"""hpmvs_level_walk_batch -- the wave walk of an extend level inside ONE device call -- against the host walk.

  * The levels: two scenes are prepared identically; one level runs with the host walk (frontier._walk) on the first and with
    device_walk=True on the second.  Compared as bytes: stage, counts, accepted, waves, deferred_per_wave, border, leaf keys,
    occupancy / trees and every level of every view's depth map.  configs[0] (60 parents, 360 candidates), a 12-view scene (150
    parents, 900 candidates), that scene through filter_extend_level with multi-patch leaves (events), and extend_level_tree /
    extend_level_forest on a partition of configs[0]'s seed tree.
  * The entry itself against _walk driven by api.depth_gates_batch / api.depth_ops_batch on a queue of 130 items that all sit
    on the same few cells: long chains inside a wave, many waves.
  * Host and device pointers; n == 0, events only, unrefined candidates only; every refusal with the outputs and the maps untouched."""
import copy
import ctypes as C

import numpy as np
import pytest

from level_walk_ref import BORDER, EVENT, HAS_PRE, PRE_TAKEN, REFINED

pytestmark = pytest.mark.gpu
MARGIN = 1.0


def _maps(g):
    from hpmvs_amd import api
    return {(v, l): api.depth_get_level(g, v, l) for v in range(g.n_views) for l in range(g.view_levels[v])}


def _restore(g, maps):
    from hpmvs_amd import api
    for (v, l), m in maps.items():
        api.depth_set_level(g, v, l, m)


def _same_maps(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), (what, "depth map", key, int((a[key] != b[key]).sum()))


def _same_level(A, B, what):
    """Two LevelResults, field by field, as bytes."""
    assert A.stage.tobytes() == B.stage.tobytes(), (what, np.nonzero(A.stage != B.stage)[0][:10])
    assert A.counts.tobytes() == B.counts.tobytes(), (what, np.nonzero((A.counts != B.counts).any(axis=1))[0][:10])
    assert A.accepted == B.accepted and A.waves == B.waves and A.deferred_per_wave == B.deferred_per_wave, \
        (what, A.waves, B.waves, A.deferred_per_wave, B.deferred_per_wave)
    assert A.border == B.border and A.leaf_key == B.leaf_key and A.tree.tobytes() == B.tree.tobytes(), what
    for name in ("center", "normal", "scale", "n_images", "images", "stage"):
        assert getattr(A.candidates, name).tobytes() == getattr(B.candidates, name).tobytes(), (what, name)


@pytest.fixture(scope="module")
def scenes12():
    from hpmvs_amd import api, synth
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    a, b = api.Scene(scene, device=0), api.Scene(scene, device=0)
    yield scene, a, b
    a.close(); b.close()


@pytest.fixture(scope="module")
def scenes3(tiny_scene):
    from hpmvs_amd import api
    a, b = api.Scene(tiny_scene, device=0), api.Scene(tiny_scene, device=0)
    yield tiny_scene, a, b
    a.close(); b.close()


def _parents(g, seeds, n_parents):
    from hpmvs_amd import api
    b0 = api.Batch.from_seeds(seeds)
    api.optimize_batch(g, b0)
    keep = np.nonzero(b0.ok)[0][:n_parents]
    parents = api.Batch(b0.center[keep], b0.normal[keep], b0.scale[keep], b0.n_images[keep], b0.images[keep])
    parents.ok[:] = 1
    return parents, float(np.float32(2.0 * np.median(parents.scale) / 0.9))


def _enter(g, P):
    from hpmvs_amd import api
    api.depth_reset(g)
    P.ok[:] = 1
    api.set_depths_batch(g, P)


def _extend_both(tag, a, b, seeds, n_parents, min_waves):
    from hpmvs_amd import api, frontier
    parents, width = _parents(a, seeds, n_parents)
    occ0 = {frontier.cell_key(parents.center[k], width) for k in range(parents.n)}
    out = []
    for g, dev in ((a, False), (b, True)):
        _enter(g, parents)
        occ = set(occ0)
        out.append((frontier.extend_level(g, parents, width, occ, MARGIN, 0, device_walk=dev), occ, _maps(g)))
    (H, occ_h, maps_h), (D, occ_d, maps_d) = out
    assert H.waves >= min_waves and len(H.stage) == 6 * n_parents, (tag, H.waves)   # (the host walk: the level interacts through the maps)
    _same_level(H, D, tag)
    assert occ_h == occ_d, tag
    _same_maps(maps_h, maps_d, tag)
    print("level_walk", tag, "candidates", len(H.stage), "accepted", len(H.accepted), "waves", H.waves, "deferred", H.deferred_per_wave,
          "device rounds / most in a wave / in-order passes", api.last_level_walk(b))
    return H


def test_configs0_level_equals_the_host_walk(scenes3, tiny_seeds):
    _, a, b = scenes3
    _extend_both("configs0", a, b, tiny_seeds, 60, 2)


def test_12_view_level_equals_the_host_walk(scenes12):
    from hpmvs_amd import synth
    scene, a, b = scenes12
    H = _extend_both("12v", a, b, synth.make_seeds(scene, 600, start_level=2), 150, 2)
    assert len(H.stage) == 900


def test_filter_extend_level_with_events_equals_the_host_walk(scenes12):
    from hpmvs_amd import api, frontier
    from test_gpu_filter_level import _grid_cells, _survivors, _width
    scene, a, b = scenes12
    R = _survivors(scene, a, 900, 0)
    width = _width(R, 3.0)
    P, cs, occ0 = _grid_cells(R, width)
    out = []
    for g, dev in ((a, False), (b, True)):
        _enter(g, P)
        occ = set(occ0)
        F, L = frontier.filter_extend_level(g, P, cs, width, occ, margin=MARGIN, device_walk=dev)
        out.append((F, L, occ, _maps(g)))
    (Fh, H, occ_h, maps_h), (Fd, D, occ_d, maps_d) = out
    assert int(Fh.removed.sum()) >= 1 and H.waves >= 2      # (at least one event is in the queue)
    assert Fh.keep.tobytes() == Fd.keep.tobytes() and Fh.removed.tobytes() == Fd.removed.tobytes()
    _same_level(H, D, "filter_extend 12v")
    assert occ_h == occ_d
    _same_maps(maps_h, maps_d, "filter_extend 12v")
    print("level_walk filter_extend 12v: cells", len(cs) - 1, "events", int(Fh.removed.sum()), "waves", H.waves, "deferred", H.deferred_per_wave,
          "device rounds / most in a wave / in-order passes", api.last_level_walk(b))


def test_tree_and_forest_levels_equal_the_host_walk(scenes3):
    """configs[0]'s seed tree, its partition into small subtrees (min_split_leaves = 4), and on each of the two lowest levels
    extend_level_tree on the subtree with the most parents and extend_level_forest over all of them."""
    from hpmvs_amd import api, frontier
    from hpmvs_amd.frontier import key_depth
    from test_gpu_extend_level_tree import CASES, level_parents, make_seed_batch
    scene, a, b = scenes3
    seeds = make_seed_batch(scene, CASES["configs0"]["groups"])
    api.optimize_batch(a, seeds)
    k = np.nonzero(seeds.ok)[0]
    R = api.Batch(seeds.center[k], seeds.normal[k], seeds.scale[k], seeds.n_images[k], seeds.images[k])
    state = []
    for g in (a, b):
        R.ok[:] = 1
        api.depth_reset(g)
        T = frontier.seed_tree(g, R, patch_init_maxlevel=CASES["configs0"]["maxlevel"], set_depths=True)
        O = frontier.Octree.from_seed_tree(T)
        P = frontier.partition(g, O, min_trees=8, min_split_leaves=4)
        state.append((T, O, P, _maps(g)))
    (T, O, P, start), (_, _, Pb, start_b) = state
    assert len(P.trees) >= 3 and len(Pb.trees) == len(P.trees)
    _same_maps(start, start_b, "seed tree")
    stages = []
    for depth in sorted({key_depth(k) for k in O.leaves})[:2]:
        width = np.float32(O.cell(next(k for k in O.leaves if key_depth(k) == depth))[1])
        per_tree = []
        for t, S in enumerate(P.trees):
            d = depth - key_depth(int(P.root_key[t]))
            per_tree.append(level_parents(S, T, d)[1] if d >= 1 else [])
        rows = lambda leaves: frontier._rows(R, [int(T.rows[T.cell_start[l]]) for l in leaves])
        # one tree: the one with the most parents on this level
        best = max(range(len(per_tree)), key=lambda t: len(per_tree[t]))
        res = []
        for g, trees, dev in ((a, P.trees, False), (b, Pb.trees, True)):
            _restore(g, start)
            tree = copy.deepcopy(trees[best])
            L = frontier.extend_level_tree(g, rows(per_tree[best]), width, tree, MARGIN, 0, device_walk=dev)
            res.append((L, tree, _maps(g)))
        _same_level(res[0][0], res[1][0], ("tree", depth))
        assert res[0][1].branches == res[1][1].branches and set(res[0][1].leaves) == set(res[1][1].leaves)
        _same_maps(res[0][2], res[1][2], ("tree", depth))
        stages += res[0][0].stage.tolist()
        # every tree at once
        leaves = [l for per in per_tree for l in per]
        tree_of = np.repeat(np.arange(len(per_tree), dtype=np.int32), [len(per) for per in per_tree])
        res = []
        for g, trees, dev in ((a, P.trees, False), (b, Pb.trees, True)):
            _restore(g, start)
            forest = copy.deepcopy(trees)
            L = frontier.extend_level_forest(g, rows(leaves), tree_of, width, forest, MARGIN, 0, device_walk=dev)
            res.append((L, forest, _maps(g)))
        _same_level(res[0][0], res[1][0], ("forest", depth))
        for ta, tb in zip(res[0][1], res[1][1]):
            assert ta.branches == tb.branches and set(ta.leaves) == set(tb.leaves)
        _same_maps(res[0][2], res[1][2], ("forest", depth))
        H = res[0][0]
        stages += H.stage.tolist()
        print("level_walk forest depth", depth, "trees", len(P.trees), "candidates", len(H.stage), "waves", H.waves, "stages",
              {int(s): int(c) for s, c in zip(*np.unique(H.stage, return_counts=True))}, "device rounds / most / in-order passes",
              api.last_level_walk(b))
    assert 27 in stages and 26 in stages, sorted(set(stages))      # (the host walk's: a border candidate and a refusal by addConditional)


# ---- the entry itself

def _tokens(g, fp, is_ev):
    """frontier._level's token sets from ONE hpmvs_level_conflicts_batch: (read_tok, write_tok) per node."""
    from hpmvs_amd import api
    read_tok, write_tok = [set() for _ in range(fp.n)], [set() for _ in range(fp.n)]
    flow_off, flow_adj, anti_off, anti_adj = api.level_conflicts(g, fp, is_ev)
    for i in range(fp.n):
        for j in flow_adj[flow_off[i]:flow_off[i + 1]].tolist():
            if is_ev[i]:
                write_tok[i].add(("ww", j, i)); write_tok[j].add(("ww", j, i))
            else:
                write_tok[j].add(("rw", j, i)); read_tok[i].add(("rw", j, i))
        for j in anti_adj[anti_off[i]:anti_off[i + 1]].tolist():
            if is_ev[j]:
                write_tok[i].add(("ww", i, j)); write_tok[j].add(("ww", i, j))
            else:
                write_tok[i].add(("rw", i, j)); read_tok[j].add(("rw", i, j))
    return read_tok, write_tok


@pytest.fixture(scope="module")
def dense_queue(scenes3, tiny_seeds):
    """130 items, copies of three accepted candidates of the configs[0] level with distinct keys, every third an event on one of
    them: every item shares its cells with a third of the others.  Returns (items batch, flags, pre, post, start maps)."""
    from hpmvs_amd import api, frontier
    _, a, _ = scenes3
    parents, width = _parents(a, tiny_seeds, 60)
    _enter(a, parents)
    start = _maps(a)
    L = frontier.extend_level(a, parents, width, {frontier.cell_key(parents.center[k], width) for k in range(parents.n)}, MARGIN, 0)
    assert len(L.accepted) >= 3
    src = [L.accepted[0], L.accepted[len(L.accepted) // 2], L.accepted[-1]]
    n = 130
    rows = [src[(i // 3 + i) % 3] for i in range(n)]
    items = frontier._rows(L.candidates, rows)
    flags = np.array([EVENT if i % 3 == 2 else REFINED | HAS_PRE for i in range(n)], np.uint8)
    pre = np.arange(n, dtype=np.uint64) + np.uint64(1000)
    post = np.arange(n, dtype=np.uint64) + np.uint64(5000)
    return items, flags, pre, post, start


def _walk_on_host(g, items, flags, pre, post):
    """frontier._walk over the items, the device behind api.depth_gates_batch / api.depth_ops_batch."""
    from hpmvs_amd import api, frontier
    n = items.n
    is_ev = (flags & EVENT) != 0
    refined = (flags & REFINED) != 0
    nodes = [i for i in range(n) if is_ev[i] or refined[i]]
    node_of = {i: k for k, i in enumerate(nodes)}
    read_tok, write_tok = _tokens(g, frontier._rows(items, nodes), is_ev[nodes].astype(np.uint8))
    queue = [("e", i) if is_ev[i] else ("c", i) for i in range(n)]      # (events and candidates both named by their item)
    ev_cells = {i: write_tok[node_of[i]] for i in range(n) if is_ev[i]}
    stage, counts = np.zeros(n, np.int32), np.full((n, 3), -1, np.int32)

    def gates(todo):
        v, b, f = api.depth_gates_batch(g, frontier._rows(items, todo), MARGIN, 0)
        return [(int(v[k]), int(b[k]), int(f[k])) for k in range(len(todo))]

    def apply(ops):
        batch = frontier._rows(items, [t for _, t in ops])
        batch.ok[:] = 1
        api.depth_ops_batch(g, batch, np.array([kind == "e" for kind, _ in ops], np.uint8))

    occupied = set()
    accepted, waves, deferred = frontier._walk(queue, {i: int(pre[i]) for i in range(n)}, {i: int(post[i]) for i in range(n)}, refined,
                                               items.n_images, lambda t: read_tok[node_of[t]], lambda t: write_tok[node_of[t]], ev_cells,
                                               occupied, 3, stage, counts, gates, apply)
    return stage, counts, accepted, waves, deferred


def test_the_entry_equals_the_walk_on_a_dense_queue(scenes3, dense_queue):
    from hpmvs_amd import api
    _, a, b = scenes3
    items, flags, pre, post, start = dense_queue
    _restore(a, start); _restore(b, start)
    stage, counts, accepted, waves, deferred = _walk_on_host(a, items, flags, pre, post)
    st, cnt, acc, wave, n_waves = api.level_walk(b, items, flags, None, pre, post, MARGIN, 0, stage=np.zeros(items.n, np.int32))
    rounds = api.last_level_walk(b)
    print("level_walk dense queue: items", items.n, "waves", waves, "deferred", deferred, "accepted", len(accepted),
          "device rounds / most in a wave / in-order passes", rounds)
    assert waves >= 5 and n_waves == waves
    assert st.tobytes() == stage.tobytes() and cnt.tobytes() == counts.tobytes()
    assert [int(i) for _, i in sorted((wave[i], i) for i in np.nonzero(acc)[0])] == accepted
    assert [int((wave > w + 1).sum()) for w in range(n_waves)] == deferred and wave.min() >= 1
    _same_maps(_maps(a), _maps(b), "dense queue")


def _device_call(g, items, flags, sets, pre, post, stage0):
    """The call with device pointers throughout -> (rc, stage, counts, accepted, wave, n_waves)."""
    import torch
    from hpmvs_amd import api
    dev = "cuda"
    t = {name: torch.from_numpy(getattr(items, name)).to(dev) for name in ("center", "normal", "scale", "n_images", "images")}
    pb = api.PatchBatch()
    pb.n, pb.max_images = items.n, items.max_images
    for name, x in t.items():
        setattr(pb, name, x.data_ptr())
    tf = torch.from_numpy(flags).to(dev)
    ts = None if sets is None else torch.from_numpy(sets).to(dev)
    tp, tq = torch.from_numpy(pre.view(np.int64)).to(dev), torch.from_numpy(post.view(np.int64)).to(dev)
    n = items.n
    tst = torch.from_numpy(stage0.astype(np.int32)).to(dev)
    tc = torch.full((n, 3), 77, dtype=torch.int32, device=dev)
    ta = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    tw = torch.full((n,), 77, dtype=torch.int32, device=dev)
    nw = C.c_int32(-7)
    o = api.default_options()
    torch.cuda.synchronize()
    rc = api.lib().hpmvs_level_walk_batch(g.h, C.byref(o), C.byref(pb), tf.data_ptr(), None if ts is None else ts.data_ptr(), tp.data_ptr(),
                                          tq.data_ptr(), MARGIN, 0, tst.data_ptr(), tc.data_ptr(), ta.data_ptr(), tw.data_ptr(), C.byref(nw), 1, None)
    torch.cuda.synchronize()
    return rc, tst.cpu().numpy(), tc.cpu().numpy(), ta.cpu().numpy(), tw.cpu().numpy(), nw.value


def test_host_and_device_pointers_give_the_same_bytes(scenes3, dense_queue):
    from hpmvs_amd import api
    _, a, b = scenes3
    items, flags, pre, post, start = dense_queue
    n = 40                                  # (a prefix of the queue: the same chains, fewer waves)
    from hpmvs_amd import frontier
    part = frontier._rows(items, np.arange(n))
    sets = (np.arange(n) % 2).astype(np.int32)
    _restore(a, start); _restore(b, start)
    st, cnt, acc, wave, n_waves = api.level_walk(a, part, flags[:n], sets, pre[:n], post[:n], MARGIN, 0, stage=np.zeros(n, np.int32))
    rc, dst, dcnt, dacc, dwave, dn = _device_call(b, part, flags[:n].copy(), sets, pre[:n].copy(), post[:n].copy(), np.zeros(n, np.int32))
    assert rc == 0 and dn == n_waves and n_waves >= 2
    assert (dst.tobytes(), dcnt.tobytes(), dacc.tobytes(), dwave.tobytes()) == (st.tobytes(), cnt.tobytes(), acc.tobytes(), wave.tobytes())
    _same_maps(_maps(a), _maps(b), "pointer forms")


def test_empty_queues_events_only_and_unrefined_only(scenes3, dense_queue):
    from hpmvs_amd import api, frontier
    _, a, b = scenes3
    items, flags, pre, post, start = dense_queue
    _restore(a, start)
    none = frontier._rows(items, np.zeros(0, np.int64))
    st, cnt, acc, wave, n_waves = api.level_walk(a, none, np.zeros(0, np.uint8), None, np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    assert n_waves == 0 and len(st) == 0
    _same_maps(_maps(a), start, "n == 0")
    # events only: one wave applies them all -- the maps equal ONE ordered depth update
    ev = frontier._rows(items, np.nonzero(flags & EVENT)[0][:7])
    st, cnt, acc, wave, n_waves = api.level_walk(a, ev, np.full(7, EVENT, np.uint8), None, np.zeros(7, np.uint64), np.zeros(7, np.uint64),
                                                 stage=np.full(7, 5, np.int32))
    assert n_waves == 1 and (wave == 1).all() and not acc.any() and (cnt == -1).all() and (st == 5).all()
    _restore(b, start)
    ev.ok[:] = 1
    api.depth_ops_batch(b, ev, np.ones(7, np.uint8))
    _same_maps(_maps(a), _maps(b), "events only")
    # unrefined candidates only (their rows are not read: NaN): preset stages stay, a taken leaf is a 20, nothing is written
    _restore(a, start)
    un = frontier._rows(items, np.arange(5))
    un.center[:] = np.nan; un.normal[:] = np.nan; un.scale[:] = np.nan; un.n_images[:] = -5
    fl = np.array([HAS_PRE, 0, HAS_PRE | PRE_TAKEN, HAS_PRE, 0], np.uint8)
    st, cnt, acc, wave, n_waves = api.level_walk(a, un, fl, None, np.array([1, 1, 2, 1, 9], np.uint64), np.zeros(5, np.uint64),
                                                 stage=np.array([1, 2, 3, 4, 5], np.int32))
    assert n_waves == 1 and st.tolist() == [1, 2, 20, 4, 5] and not acc.any() and (cnt == -1).all() and (wave == 1).all()
    _same_maps(_maps(a), start, "unrefined only")


def _raw_call(g, items, flags, sets, pre, post, out, o=None, n=None, max_images=None, null=()):
    """The C entry with host pointers; out = (stage, counts, accepted, wave) arrays; null: argument names passed as NULL."""
    from hpmvs_amd import api
    pb = items.c_struct()
    if n is not None:
        pb.n = n
    if max_images is not None:
        pb.max_images = max_images
    args = dict(flags=flags, set=sets, pre=pre, post=post, stage=out[0], counts=out[1], accepted=out[2], wave=out[3])
    p = {k: (None if (k in null or v is None) else v.ctypes.data) for k, v in args.items()}
    nw = C.c_int32(-7)
    o = o or api.default_options()
    rc = api.lib().hpmvs_level_walk_batch(g.h, C.byref(o), None if "items" in null else C.byref(pb), p["flags"], p["set"], p["pre"], p["post"],
                                          MARGIN, 0, p["stage"], p["counts"], p["accepted"], p["wave"], None if "n_waves" in null else C.byref(nw),
                                          0, None)
    return rc


def test_every_refusal_leaves_outputs_and_maps_untouched(scenes3, tiny_scene, dense_queue):
    from hpmvs_amd import api, frontier
    _, a, _ = scenes3
    items, flags, pre, post, start = dense_queue
    n = 12
    part = frontier._rows(items, np.arange(n))
    fl, pr, po = flags[:n].copy(), pre[:n].copy(), post[:n].copy()
    _restore(a, start)

    def poisoned():
        return (np.full(n, 77, np.int32), np.full((n, 3), 77, np.int32), np.full(n, 77, np.uint8), np.full(n, 77, np.int32))

    def refused(code, what, **kw):
        out = poisoned()
        args = dict(items=part, flags=fl, sets=None, pre=pr, post=po)
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        rc = _raw_call(a, args["items"], args["flags"], args["sets"], args["pre"], args["post"], out, **kw)
        assert rc == code, (what, rc, api.lib().hpmvs_last_error())
        assert all((x == 77).all() for x in out), what
        _same_maps(_maps(a), start, what)

    for name in ("items", "flags", "pre", "post", "stage", "counts", "accepted", "wave", "n_waves"):
        refused(-2, "null " + name, null=(name,))
    for bad in (EVENT | REFINED, EVENT | BORDER, 64, 128 | REFINED):
        f2 = fl.copy(); f2[5] = bad
        refused(-2, ("flag byte", bad), flags=f2)
    refused(-2, "a negative set", sets=np.where(np.arange(n) == 3, -1, 0).astype(np.int32))
    refused(-2, "max_images 0", max_images=0)
    refused(-2, "max_images beyond HPMVS_MAX_IMAGES", max_images=api.MAX_IMAGES + 1)
    refused(-2, "n * max_images >= 2^28", n=(1 << 28) // part.max_images + 1)     # (refused before any array is read)
    refused(-2, "negative n", n=-1)
    o = api.default_options(); o.MIN_IMAGES_PER_PATCH = 0
    refused(-2, "MIN_IMAGES_PER_PATCH 0", o=o)
    # a scene without depth maps: HPMVS_ERR_STATE
    bare = api.Scene(tiny_scene, device=0)
    try:
        out = poisoned()
        assert _raw_call(bare, part, fl, None, pr, po, out) == -3 and all((x == 77).all() for x in out)
    finally:
        bare.close()
    # the graph's 2^30-pair refusal: 32768 refined copies of one patch, every one reading what every other writes
    big = 32768
    cand = int(np.nonzero((flags & REFINED) != 0)[0][0])
    many = frontier._rows(items, np.full(big, cand))
    out = (np.full(big, 77, np.int32), np.full((big, 3), 77, np.int32), np.full(big, 77, np.uint8), np.full(big, 77, np.int32))
    rc = _raw_call(a, many, np.full(big, REFINED, np.uint8), None, np.zeros(big, np.uint64), np.arange(big, dtype=np.uint64), out)
    assert rc == -3 and b"2^30" in api.lib().hpmvs_last_error(), (rc, api.lib().hpmvs_last_error())
    assert all((x == 77).all() for x in out)
    _same_maps(_maps(a), start, "2^30 pairs")
    # ... and after all that the call still works
    st, cnt, acc, wave, n_waves = api.level_walk(a, part, fl, None, pr, po, stage=np.zeros(n, np.int32))
    assert n_waves >= 1 and wave.min() >= 1
