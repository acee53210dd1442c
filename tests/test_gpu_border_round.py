"""A round across subtree boundaries on batched calls -- extend_level_tree on subtree A, route_border over every subtree,
insert_border into each target, a second extend_level_tree on subtree B -- against the sequential loop on pointer trees
(tests/octree_tree_ref.py: sequential_extend for the levels, and CellProcessor::distributeBorderCell / processBorderCellQueue
restated here over Tree.contains, Tree.add_conditional and the oracle's orc_set_depths), from seeds through seed_tree, on
BASELINE configs[0] and on the 12-view scene of the level tests.  Everything is exact: the tree every border patch goes to, the
accepted patches and their order, leaf keys and node levels, the final branch and leaf sets of every subtree, every depth-map
cell; and for the second level every stage, count, accepted candidate and border patch.

A and B are siblings, chosen on the sequential reference alone: A is the first subtree (most leaves first) whose lowest level
sends border patches into a sibling, B the sibling that accepts most of them.  The second level runs on the node level of B that
holds most of the inserted border leaves, over every nonempty leaf of that level: the inserted leaves are parents there, and
nonempty leaves to the pre-gate of their neighbours' candidates."""
import numpy as np
import pytest

import filter_ref as fr
import octree_tree_ref as otr

pytestmark = pytest.mark.gpu
MARGIN = 1.0
f32 = np.float32

# scene -> seed groups (count, start level, seed offset), PATCH_INIT_MAXLEVEL, depth of the subtrees' roots: as in
# tests/test_gpu_extend_level_tree.py
CASES = {
    "configs0": dict(views=3, groups=((300, 2, 11), (200, 3, 12)), maxlevel=9, sub_depth=1),
    "12v": dict(views=12, groups=((500, 2, 0), (300, 3, 1)), maxlevel=9, sub_depth=2),
}


def _seed_batch(scene, groups):
    from hpmvs_amd import api, synth
    parts = [api.Batch.from_seeds(synth.make_seeds(scene, n, start_level=lvl, seed=synth.SEED + off)) for n, lvl, off in groups]
    M = max(b.max_images for b in parts)
    pad = lambda a: np.pad(a, ((0, 0), (0, M - a.shape[1])), constant_values=-1)
    return api.Batch(*[np.concatenate([getattr(b, f) if f != "images" else pad(b.images) for b in parts])
                       for f in ("center", "normal", "scale", "n_images", "images")])


def _patches(B, rows):
    from oracle import oracle as orc
    return (orc.Patch * len(rows))(*[fr.oracle_patch(B, int(r))[0] for r in rows])


def _array(patches):
    from oracle import oracle as orc
    return (orc.Patch * len(patches))(*patches)


def _maps_equal(g, OD):
    from hpmvs_amd import api
    for v in range(g.n_views):
        for l in range(g.view_levels[v]):
            a, b = api.depth_level(g, v, l), OD.level(v, l)
            if not np.array_equal(a, b):
                return (v, l, int((a != b).sum()))
    return None


def _seed_parents(S, T, depth):
    """the seed leaves of node depth `depth` of subtree S in Leaf_iterator order: the first row of each"""
    from hpmvs_amd.frontier import key_depth
    keys, rows, _, _ = S.leaf_table()
    return [int(T.rows[T.cell_start[int(rows[i])]]) for i, k in enumerate(keys) if key_depth(int(k)) == depth]


def _seed_maps(oscene, R, T):
    from oracle import oracle as orc
    OD = orc.OracleDepths(oscene)
    for i in T.rows:
        OD.set_depths(fr.oracle_patch(R, int(i))[0])
    return OD


def _pointer_trees(subs):
    return [otr.tree_from_keys(S.root_center, S.root_width, S.branches, S.leaves) for S in subs]


def _reference_round(oscene, R, T, subs, a, cache):
    """extend on subtree a's lowest level, then distributeBorderCell / processBorderCellQueue over all subtrees, sequentially.
    -> dict(ref (the level), width, parents, trees, depths, target [border], accepted {tree: [(row of border, key, depth)]},
    patches (the border candidates as oracle patches))"""
    from hpmvs_amd.frontier import key_depth
    TR = _pointer_trees(subs)
    OD = _seed_maps(oscene, R, T)
    S = subs[a]
    depth = min(key_depth(k) for k in S.leaves)
    parents = _seed_parents(S, T, depth)
    width = S.cell(next(k for k in S.leaves if key_depth(k) == depth))[1]
    keys = [("seed", int(r)) for r in parents]
    ref = otr.sequential_extend(oscene, OD, _patches(R, parents), width, TR[a], MARGIN, 0, cache=cache, cache_keys=keys)
    _, refined = otr.expand_six(oscene, _patches(R, parents), width, None, cache, keys)
    patches = [refined[t] for t in ref["border"]]
    target = []
    for q in patches:                                           # distributeBorderCell: the first processor whose root contains it
        c = np.array(q.center[:3], f32)
        target.append(next((k for k, tr in enumerate(TR) if tr.contains(c)), -1))
    accepted = {}
    for k in sorted(set(target) - {-1}):                        # processBorderCellQueue of every processor that got some
        accepted[k] = []
        for j, q in enumerate(patches):
            if target[j] != k:
                continue
            c = np.array(q.center[:3], f32)
            leaf = TR[k].add_conditional(c, ("border", j), f32(float(f32(q.scale)) * 2.0))
            if leaf is not None:
                OD.set_depths(q)
                accepted[k].append((j, TR[k].key(leaf), TR[k].depth(leaf)))
    return dict(ref=ref, width=width, parents=parents, trees=TR, depths=OD, target=target, accepted=accepted, patches=patches)


_state = {}


def _setup(tag):
    """scene, GPU scene, oracle scene, refined survivors, seed tree, subtree keys and the reference round, once per module"""
    if tag in _state:
        return _state[tag]
    from hpmvs_amd import api, frontier, synth
    from oracle import oracle as orc
    c = CASES[tag]
    scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    b = _seed_batch(scene, c["groups"])
    api.optimize_batch(g, b)
    k = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
    R.ok[:] = 1
    orc.build()
    o = orc.OracleScene(scene)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=False)   # (floors R.scale in place: idempotent)
    O = frontier.Octree.from_seed_tree(T)
    roots = sorted(k for k in O.branches if frontier.key_depth(k) == c["sub_depth"])
    subs = [O.subtree(k) for k in roots]
    cache, chosen = {}, None
    for a in sorted(range(len(roots)), key=lambda i: -len(subs[i].leaves)):
        rr = _reference_round(o, R, T, subs, a, cache)
        siblings = [k for k in rr["accepted"] if k != a and roots[k] >> 3 == roots[a] >> 3 and rr["accepted"][k]]
        if siblings:
            chosen = (a, max(siblings, key=lambda k: len(rr["accepted"][k])), rr)
            break
    assert chosen is not None, "no subtree of the scene sends a border patch into a sibling"
    _state[tag] = dict(g=g, o=o, R=R, roots=roots, a=chosen[0], b=chosen[1], rr=chosen[2], cache=cache, maxlevel=c["maxlevel"])
    return _state[tag]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _state.values():
        s["g"].close()
    _state.clear()


@pytest.mark.parametrize("tag", list(CASES))
def test_border_round_equals_the_sequential_loop(tag):
    from hpmvs_amd import api, frontier
    st = _setup(tag)
    g, R, rr, a, b = st["g"], st["R"], st["rr"], st["a"], st["b"]
    api.depth_reset(g)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=st["maxlevel"], set_depths=True)
    O = frontier.Octree.from_seed_tree(T)
    subs = [O.subtree(k) for k in st["roots"]]
    ref = rr["ref"]

    # the level on A
    L = frontier.extend_level_tree(g, frontier._rows(R, rr["parents"]), rr["width"], subs[a], MARGIN, 0)
    assert len(ref["border"]) > 0 and L.border == ref["border"] and L.accepted == ref["accepted"]
    assert np.array_equal(L.stage, ref["stage"])

    # route and insert
    border = frontier._rows(L.candidates, L.border)
    priority = np.arange(border.n, dtype=f32) * f32(0.5)
    tree = frontier.route_border(g, subs, border.center)
    assert tree.tolist() == rr["target"]
    inserted = {}
    for k in sorted(set(tree.tolist()) - {-1}):
        rows = np.nonzero(tree == k)[0]
        res = frontier.insert_border(g, subs[k], frontier._rows(border, rows), priority[rows], rows=[("border", int(j)) for j in rows])
        inserted[k] = res
        want = rr["accepted"][k]
        assert [int(rows[i]) for i in res.accepted] == [j for j, _, _ in want], (tag, k)
        assert res.leaf_key.tolist() == [key for _, key, _ in want], (tag, k)
        assert res.node_level.tolist() == [d + frontier.key_depth(st["roots"][k]) for _, _, d in want], (tag, k)
        assert not res.flatness.any() and res.priority.tobytes() == priority[rows][res.accepted].tobytes()
    assert set(inserted) == set(rr["accepted"])
    for k, S in enumerate(subs):
        branches, leaves, _ = rr["trees"][k].key_sets()
        assert S.branches == branches and set(S.leaves) == set(leaves), (tag, k)
    bad = _maps_equal(g, rr["depths"])
    assert bad is None, (tag, bad)
    summary = dict(A=oct(st["roots"][a]), B=oct(st["roots"][b]), border=border.n, dropped=int((tree < 0).sum()),
                   accepted={oct(st["roots"][k]): len(v) for k, v in rr["accepted"].items()})

    # a second level, on B: the node level that holds most of the inserted leaves, every nonempty leaf of it a parent
    S, TR, OD = subs[b], rr["trees"][b], rr["depths"]
    depths = [frontier.key_depth(key) for _, key, _ in rr["accepted"][b]]
    depth = max(sorted(set(depths)), key=depths.count)
    keys, rows, _, _ = S.leaf_table()
    level = [i for i, key in enumerate(keys) if frontier.key_depth(int(key)) == depth]
    assert any(isinstance(rows[i], tuple) for i in level)
    both = frontier._concat([frontier._rows(R, np.arange(R.n), border.max_images), frontier._rows(border, np.arange(border.n), R.max_images)])
    pick = [R.n + rows[i][1] if isinstance(rows[i], tuple) else int(T.rows[T.cell_start[int(rows[i])]]) for i in level]
    oracle_parents = _array([rr["patches"][p - R.n] if p >= R.n else fr.oracle_patch(R, p)[0] for p in pick])
    width = S.cell(int(keys[level[0]]))[1]
    ref2 = otr.sequential_extend(st["o"], OD, oracle_parents, width, TR, MARGIN, 0, cache=st["cache"],
                                 cache_keys=[("border", tag, p - R.n) if p >= R.n else ("seed", p) for p in pick])
    L2 = frontier.extend_level_tree(g, frontier._rows(both, pick), width, S, MARGIN, 0)
    diff = np.nonzero(L2.stage != ref2["stage"])[0]
    assert len(diff) == 0, (tag, diff[:10], L2.stage[diff[:10]], ref2["stage"][diff[:10]])
    assert np.array_equal(L2.counts, ref2["counts"]) and L2.accepted == ref2["accepted"] and L2.border == ref2["border"]
    branches, leaves, _ = TR.key_sets()
    assert S.branches == branches and set(S.leaves) == set(leaves), (tag, "second level")
    bad = _maps_equal(g, OD)
    assert bad is None, (tag, "second level", bad)
    summary.update(second=dict(depth=depth, parents=len(pick), inserted_parents=sum(p >= R.n for p in pick), accepted=len(L2.accepted),
                               pre_gated=int((ref2["stage"] == 20).sum()), tally={k: int(v) for k, v in ref2["tally"].items()}))
    print("border_round", tag, summary)
    assert summary["second"]["inserted_parents"] >= 1 and summary["second"]["pre_gated"] >= 1
