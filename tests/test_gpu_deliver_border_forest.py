"""frontier.deliver_border_forest -- ONE hpmvs_border_forest_batch for a round's border queue -- against today's per-tree path
(one route_border, then one insert_border per destination tree, as INTEGRATION.md had it) on a twin scene.  On BASELINE configs[0]
with the subtrees at depth 1 and on the 12-view scene with the subtrees at depth 2, as tests/test_gpu_border_round.py builds them:
one extend_level_forest over the lowest populated level of every subtree, the delivery of its border patches, then a second
extend_level_forest over the same level, whose leaves now hold the first level's and the border's patches.  Equal on both sides:
every tree's branch and leaf sets, the accepted rows, keys, node levels and priorities, every depth-map cell, and of the second
level every stage, the accepted set and the border set."""
import numpy as np
import pytest

from test_gpu_border_round import CASES, _seed_batch

pytestmark = pytest.mark.gpu
MARGIN = 1.0
f32 = np.float32


def _side(scene, R, maxlevel, sub_depth):
    """a GPU scene with the seeds' depths, the seed tree and its subtrees"""
    from hpmvs_amd import api, frontier
    g = api.Scene(scene, device=0)
    api.depth_reset(g)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=maxlevel, set_depths=True)
    O = frontier.Octree.from_seed_tree(T)
    roots = sorted(k for k in O.branches if frontier.key_depth(k) == sub_depth)
    return g, T, [O.subtree(k) for k in roots]


def _level_parents(subs, depth, patch_of):
    """the nonempty leaves of relative depth `depth` of every subtree, in list order: (rows of the patches, parent_tree)"""
    from hpmvs_amd import frontier
    pick, tree = [], []
    for k, S in enumerate(subs):
        keys, rows, _, _ = S.leaf_table()
        for i, key in enumerate(keys):
            if frontier.key_depth(int(key)) == depth:
                pick.append(patch_of(rows[i]))
                tree.append(k)
    return pick, np.array(tree, np.int32)


def _maps(g):
    from hpmvs_amd import api
    return [api.depth_level(g, v, l) for v in range(g.n_views) for l in range(g.view_levels[v])]


@pytest.mark.parametrize("tag", list(CASES))
def test_one_delivery_equals_route_and_insert_per_tree(tag):
    from hpmvs_amd import api, frontier, synth
    c = CASES[tag]
    scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
    g0 = api.Scene(scene, device=0)
    b = _seed_batch(scene, c["groups"])
    api.optimize_batch(g0, b)
    g0.close()
    k = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
    R.ok[:] = 1
    sides = [_side(scene, R, c["maxlevel"], c["sub_depth"]) for _ in range(2)]
    try:
        depth = min(frontier.key_depth(key) for _, _, subs in sides[:1] for S in subs for key in S.leaves)
        out = []
        for one_call, (g, T, subs) in zip((True, False), sides):
            seed_row = lambda r: int(T.rows[T.cell_start[int(r)]])
            pick, parent_tree = _level_parents(subs, depth, seed_row)
            width = next(S.cell(key)[1] for S in subs for key in S.leaves if frontier.key_depth(key) == depth)
            L = frontier.extend_level_forest(g, frontier._rows(R, pick), parent_tree, width, subs, MARGIN, 0)
            border = frontier._rows(L.candidates, L.border)
            priority = np.arange(border.n, dtype=f32) * f32(0.5)
            if one_call:
                D = frontier.deliver_border_forest(g, subs, border, priority)
                tree, acc, keys, level, prio, flat = D.tree, D.accepted, D.leaf_key, D.node_level, D.priority, D.flatness
                assert D.insertion.accepted.sum() == len(acc) and (D.insertion.tree[D.insertion.leaf_key == 0] == -1).all()
            else:
                tree = frontier.route_border(g, subs, border.center)
                got = {}
                for t in sorted(set(tree.tolist()) - {-1}):
                    rows = np.nonzero(tree == t)[0]
                    res = frontier.insert_border(g, subs[t], frontier._rows(border, rows), priority[rows], rows=[("border", int(j)) for j in rows])
                    for j, i in enumerate(res.accepted):
                        got[int(rows[i])] = (res.leaf_key[j], res.node_level[j], res.priority[j], res.flatness[j])
                acc = np.array(sorted(got), np.int64)
                keys = np.array([got[i][0] for i in acc], np.uint64)
                level = np.array([got[i][1] for i in acc], np.int32)
                prio = np.array([got[i][2] for i in acc], f32)
                flat = np.array([got[i][3] for i in acc], f32)
            sets = [(set(S.branches), set(S.leaves)) for S in subs]
            maps = [m.copy() for m in _maps(g)]
            # the second level: the same depth, whose leaves now hold seeds, the first level's candidates and border patches
            both = frontier._concat([frontier._rows(R, np.arange(R.n), L.candidates.max_images),
                                     frontier._rows(L.candidates, np.arange(L.candidates.n), R.max_images)])
            cand_of_border = {i: int(t) for i, t in enumerate(L.border)}
            patch_of = lambda r: (R.n + int(r[1]) if r[0] == "extend" else R.n + cand_of_border[int(r[1])]) if isinstance(r, tuple) else seed_row(r)
            pick2, parent_tree2 = _level_parents(subs, depth, patch_of)
            L2 = frontier.extend_level_forest(g, frontier._rows(both, pick2), parent_tree2, width, subs, MARGIN, 0)
            out.append(dict(first=(L.stage.tobytes(), list(L.accepted), list(L.border)), tree=tree.tobytes(), acc=acc.tolist(),
                            keys=keys.tolist(), level=level.tolist(), prio=prio.tobytes(), flat=flat.tobytes(), sets=sets, maps=maps,
                            pick2=pick2, second=(L2.stage.tobytes(), list(L2.accepted), list(L2.border)),
                            sets2=[(set(S.branches), set(S.leaves)) for S in subs], maps2=[m.copy() for m in _maps(g)],
                            inserted_parents=sum(p >= R.n for p in pick2), n_border=border.n))
        one, loop = out
        print("deliver_border_forest", tag, dict(border=one["n_border"], accepted=len(one["acc"]), trees=len(set(np.frombuffer(one["tree"], np.int32).tolist()) - {-1}),
                                                 second_parents=len(one["pick2"]), inserted_parents=one["inserted_parents"]))
        assert one["n_border"] >= 5 and len(one["acc"]) >= 1 and not np.frombuffer(one["flat"], f32).any()
        for name in ("first", "tree", "acc", "keys", "level", "prio", "flat", "sets", "pick2", "second", "sets2"):
            assert one[name] == loop[name], (tag, name)
        for name in ("maps", "maps2"):
            assert all(np.array_equal(a, b) for a, b in zip(one[name], loop[name])), (tag, name)
        assert one["inserted_parents"] >= 1
    finally:
        for g, _, _ in sides:
            g.close()
