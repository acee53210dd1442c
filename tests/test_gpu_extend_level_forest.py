"""frontier.extend_level_forest / filter_extend_level_forest against the per-tree loop: extend_level_tree /
filter_extend_level_tree on tree 0, then tree 1, and so on, from the same starting maps.  Scenes and seeds are those of
tests/test_gpu_extend_level_tree.py; the forests are frontier.partition(g, O, min_trees=K, min_split_leaves=4) of each scene's
seed tree with K = 8.  The extend level runs over the lowest populated node level, the filter level over the second, both
readings of abs().  Compared: stages, counts, accepted order, border list, leaf keys, every candidate's tree, every tree's branch
and leaf sets and every cell of every depth map.  `waves` is the one global walk's: printed beside the sum of the per-tree waves
and asserted to be no more.

Conditions asserted on the per-tree loop alone (test_the_per_tree_loop_shows_every_case, abs_int 0, over both scenes and both
levels; measured at K = 8: 3 and 6 trees accept on the extend level, 375 border candidates routed elsewhere, 31 losers, 36 stages):
at least 3 trees accept something; at least 1 border candidate is routed by route_border to another tree of the list; the filter
level has at least 1 loser; at least one candidate's stage differs between the loop in list order and its tree run alone from the
maps and the tree its level started with (restored with api.depth_set_level) -- the trees interact through the maps, which is what
makes the order of the concatenated queue matter.  K = 8 meets all four; it was not raised."""
import copy

import numpy as np
import pytest

from test_gpu_extend_level_tree import CASES, MARGIN, _setup, _state, level_parents

pytestmark = pytest.mark.gpu
f32 = np.float32
K, MIN_SPLIT = 8, 4


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _state.values():
        s["g"].close()
    _state.clear()


def _start(tag, k=None):
    """The scene with the maps the seed tree leaves behind, the partition of the seed tree and the two levels' inputs."""
    from hpmvs_amd import api, frontier
    from hpmvs_amd.frontier import key_depth
    st = _setup(tag)
    g, R = st["g"], st["R"]
    api.depth_reset(g)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=CASES[tag]["maxlevel"], set_depths=True)
    O = frontier.Octree.from_seed_tree(T)
    P = frontier.partition(g, O, min_trees=K if k is None else k, min_split_leaves=MIN_SPLIT)
    D = sorted({key_depth(k) for k in O.leaves})[:2]
    levels = []
    for depth in D:
        width = O.cell(next(k for k in O.leaves if key_depth(k) == depth))[1]
        per_tree = []
        for k, S in enumerate(P.trees):
            d = depth - key_depth(int(P.root_key[k]))
            per_tree.append(level_parents(S, T, d)[1] if d >= 1 else [])
        levels.append(dict(depth=depth, width=f32(width), leaves=per_tree))
    return g, R, T, P, levels


def _maps(g):
    from hpmvs_amd import api
    return {(v, l): api.depth_get_level(g, v, l) for v in range(g.n_views) for l in range(g.view_levels[v])}


def _restore(g, maps):
    from hpmvs_amd import api
    for (v, l), m in maps.items():
        api.depth_set_level(g, v, l, m)


def _extend_inputs(R, T, leaves):
    from hpmvs_amd import frontier
    return frontier._rows(R, [int(T.rows[T.cell_start[l]]) for l in leaves])


def _filter_inputs(R, T, leaves):
    from hpmvs_amd import frontier
    cells = [T.rows[T.cell_start[l]:T.cell_start[l + 1]] for l in leaves]
    rows = np.concatenate(cells + [np.zeros(0, np.int64)]).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int32)
    return frontier._rows(R, rows), cs


def _one_tree(g, R, T, tree, i, lv, leaves, abs_int):
    """Level i of one tree: level 0 by extend_level_tree, level 1 by filter_extend_level_tree -> (LevelResult, FilterResult or None)"""
    from hpmvs_amd import frontier
    if i == 0:
        return frontier.extend_level_tree(g, _extend_inputs(R, T, leaves), lv["width"], tree, MARGIN, abs_int), None
    P, cs = _filter_inputs(R, T, leaves)
    F, L = frontier.filter_extend_level_tree(g, P, cs, lv["width"], tree, margin=MARGIN, abs_int=abs_int)
    return L, F


def _loop_level(g, R, T, trees, i, lv, abs_int):
    """The per-tree loop over one level, in list order -> [(tree, LevelResult, FilterResult or None)]"""
    return [(k,) + _one_tree(g, R, T, trees[k], i, lv, leaves, abs_int) for k, leaves in enumerate(lv["leaves"]) if leaves]


def _loop(g, R, T, trees, levels, abs_int):
    return [_loop_level(g, R, T, trees, i, lv, abs_int) for i, lv in enumerate(levels)]


def _forest(g, R, T, trees, levels, abs_int):
    from hpmvs_amd import frontier
    out = []
    for i, lv in enumerate(levels):
        leaves = [l for per in lv["leaves"] for l in per]
        tree_of = np.repeat(np.arange(len(trees), dtype=np.int32), [len(per) for per in lv["leaves"]])
        if i == 0:
            out.append((frontier.extend_level_forest(g, _extend_inputs(R, T, leaves), tree_of, lv["width"], trees, MARGIN, abs_int), None))
        else:
            P, cs = _filter_inputs(R, T, leaves)
            F, L = frontier.filter_extend_level_forest(g, P, cs, tree_of, lv["width"], trees, margin=MARGIN, abs_int=abs_int)
            out.append((L, F))
    return out


def _concatenated(res):
    """The per-tree results of one level as ONE result over the concatenated queue."""
    stage = np.concatenate([L.stage for _, L, _ in res])
    counts = np.concatenate([L.counts for _, L, _ in res])
    tree = np.concatenate([np.full(len(L.stage), k, np.int32) for k, L, _ in res])
    first = np.concatenate([[0], np.cumsum([len(L.stage) for _, L, _ in res])])
    accepted = [int(first[j] + t) for j, (_, L, _) in enumerate(res) for t in L.accepted]
    border = [int(first[j] + t) for j, (_, L, _) in enumerate(res) for t in L.border]
    leaf_key = {int(first[j] + t): key for j, (_, L, _) in enumerate(res) for t, key in L.leaf_key.items()}
    fields = {name: np.concatenate([getattr(L.candidates, name) for _, L, _ in res]) for name in ("center", "normal", "scale", "n_images", "stage", "ok")}
    F = None
    if res[0][2] is not None:
        rows = np.concatenate([[0], np.cumsum([len(F_.removed) for _, _, F_ in res])])
        F = dict(keep=np.concatenate([F_.keep + rows[j] for j, (_, _, F_) in enumerate(res)]), dist=np.concatenate([F_.dist for _, _, F_ in res]),
                 removed=np.concatenate([F_.removed for _, _, F_ in res]))
    return dict(stage=stage, counts=counts, tree=tree, accepted=accepted, border=border, leaf_key=leaf_key, fields=fields, F=F,
                waves=sum(L.waves for _, L, _ in res))


@pytest.mark.parametrize("abs_int", [0, 1])
@pytest.mark.parametrize("tag", list(CASES))
def test_forest_levels_equal_the_per_tree_loop(tag, abs_int):
    g, R, T, P, levels = _start(tag)
    start = _maps(g)
    trees_a, trees_b = copy.deepcopy(P.trees), copy.deepcopy(P.trees)
    loop = _loop(g, R, T, trees_a, levels, abs_int)
    maps_a = _maps(g)
    _restore(g, start)
    forest = _forest(g, R, T, trees_b, levels, abs_int)
    maps_b = _maps(g)
    for i, (res, (L, F)) in enumerate(zip(loop, forest)):
        want = _concatenated(res)
        what = (tag, abs_int, "extend" if i == 0 else "filter + extend")
        diff = np.nonzero(L.stage != want["stage"])[0]
        assert len(diff) == 0, (what, diff[:10], L.stage[diff[:10]], want["stage"][diff[:10]])
        assert np.array_equal(L.counts, want["counts"]), what
        assert L.accepted == want["accepted"] and L.border == want["border"], what
        assert L.leaf_key == want["leaf_key"] and np.array_equal(L.tree, want["tree"]), what
        for name, a in want["fields"].items():
            assert getattr(L.candidates, name).tobytes() == a.tobytes(), (what, name)
        if F is not None:
            assert np.array_equal(F.keep, want["F"]["keep"]) and F.dist.tobytes() == want["F"]["dist"].tobytes() and \
                np.array_equal(F.removed, want["F"]["removed"]), what
        print("extend_level_forest", what, "trees with parents", [k for k, _, _ in res], "candidates", len(L.stage), "accepted", len(L.accepted),
              "border", len(L.border), "waves: one walk", L.waves, "sum of the per-tree walks", want["waves"])
        assert L.waves <= want["waves"], what
    for k, (a, b) in enumerate(zip(trees_a, trees_b)):
        assert a.branches == b.branches and set(a.leaves) == set(b.leaves), (tag, abs_int, "tree", k)
    for key in maps_a:
        assert np.array_equal(maps_a[key], maps_b[key]), (tag, abs_int, "depth map", key, int((maps_a[key] != maps_b[key]).sum()))


def per_tree_conditions(k=None):
    """What the per-tree loop shows at min_trees = k (abs_int 0, both scenes, both levels)."""
    from hpmvs_amd import frontier
    accepting, routed, losers, interacting = [], 0, 0, 0
    for tag in CASES:
        g, R, T, P, levels = _start(tag, k)
        trees = copy.deepcopy(P.trees)
        for i, lv in enumerate(levels):
            start, trees_start = _maps(g), copy.deepcopy(trees)
            res = _loop_level(g, R, T, trees, i, lv, 0)
            end = _maps(g)
            if i == 0:
                accepting.append(sum(1 for _, L, _ in res if L.accepted))
            else:
                losers += sum(int(F.removed.sum()) for _, _, F in res)
            for t, L, _ in res:
                if L.border:
                    to = frontier.route_border(g, P.trees, L.candidates.center[L.border])
                    routed += int(((to >= 0) & (to != t)).sum())
                # the same tree alone, from the maps and the tree the level started with
                _restore(g, start)
                alone, _ = _one_tree(g, R, T, trees_start[t], i, lv, lv["leaves"][t], 0)
                interacting += int((alone.stage != L.stage).sum())
            _restore(g, end)
    return dict(k=K if k is None else k, accepting=accepting, routed=routed, losers=losers, interacting=interacting)


def test_the_per_tree_loop_shows_every_case():
    c = per_tree_conditions()
    print("extend_level_forest conditions: trees that accept on the extend level", c["accepting"], "border candidates routed to another tree",
          c["routed"], "filter losers", c["losers"], "stages that differ from the tree run alone", c["interacting"])
    assert max(c["accepting"]) >= 3 and c["routed"] >= 1 and c["losers"] >= 1 and c["interacting"] >= 1


def test_the_queue_must_be_the_trees_queues_in_list_order():
    from hpmvs_amd import frontier
    g, R, T, P, levels = _start("configs0")
    lv = levels[0]
    leaves = [l for per in lv["leaves"] for l in per]
    tree_of = np.repeat(np.arange(len(P.trees), dtype=np.int32), [len(per) for per in lv["leaves"]])
    assert len(np.unique(tree_of)) >= 2
    with pytest.raises(ValueError):
        frontier.extend_level_forest(g, _extend_inputs(R, T, leaves), tree_of[::-1].copy(), lv["width"], copy.deepcopy(P.trees), MARGIN, 0)
    P_, cs = _filter_inputs(R, T, leaves)
    with pytest.raises(ValueError):
        frontier.filter_extend_level_forest(g, P_, cs, tree_of[::-1].copy(), lv["width"], copy.deepcopy(P.trees), margin=MARGIN)
