"""frontier.extend_level_tree / filter_extend_level_tree against the sequential loop on the real octree
(tests/octree_tree_ref.py: sequential_extend on the pointer tree and the oracle's live maps), from seeds through seed_tree, on
BASELINE configs[0] and on the 12-view scene of the level tests: (a) the whole tree, (b) a subtree root; the two lowest
populated node levels in turn; both readings of abs().  Equal: the stage of every candidate, the counts at decision time, the
accepted order, the border list, the final branch and leaf sets, every depth-map cell.

Conditions, asserted on the REFERENCE loop alone (test_reference_loop_shows_every_case, abs_int 0), tallied over the two scenes,
whole tree and subtree, two levels each (seeds of pyramid levels 2 and 3 mixed: leaves on node levels 5 and 6):
  candidates pre-gated by a SHALLOWER nonempty leaf             193
  candidates blocked by finer structure (leaf width < w)          92
  stage 26 (addConditional refused)                              125
  stage 27 (border)                                               73
  accepted candidates whose insertion splits an empty leaf
  by two or more levels                                          109
  candidates accepted by exactly one of this loop and the
  grid-key loop (oracle.extend_round), whole trees only          681   (1 543 stage codes differ)
so the comparison cannot pass vacuously, and the last tally is the ground the grid-key level does not cover."""
import numpy as np
import pytest

import filter_ref as fr
import octree_tree_ref as otr

pytestmark = pytest.mark.gpu
MARGIN = 1.0
f32 = np.float32

# scene -> seed groups (count, start level, seed offset: seeds of two pyramid levels differ in scale by an octave, which is what
# puts the seed tree's leaves on several levels), PATCH_INIT_MAXLEVEL, depth of the subtree root (the branch of that depth with
# the most leaves)
CASES = {
    "configs0": dict(views=3, groups=((300, 2, 11), (200, 3, 12)), maxlevel=9, sub_depth=1),
    "12v": dict(views=12, groups=((500, 2, 0), (300, 3, 1)), maxlevel=9, sub_depth=2),
}


def make_seed_batch(scene, groups):
    from hpmvs_amd import api, synth
    parts = [api.Batch.from_seeds(synth.make_seeds(scene, n, start_level=lvl, seed=synth.SEED + off)) for n, lvl, off in groups]
    M = max(b.max_images for b in parts)
    pad = lambda a: np.pad(a, ((0, 0), (0, M - a.shape[1])), constant_values=-1)
    return api.Batch(*[np.concatenate([getattr(b, f) if f != "images" else pad(b.images) for b in parts])
                       for f in ("center", "normal", "scale", "n_images", "images")])


_state = {}


def _patches(B, rows):
    from oracle import oracle as orc
    return (orc.Patch * len(rows))(*[fr.oracle_patch(B, int(r))[0] for r in rows])


def subtree_root(O, depth):
    """The branch of `depth` with the most nonempty leaves below it (the root itself for depth 0)."""
    from hpmvs_amd.frontier import key_depth
    if depth == 0:
        return 1
    count = {}
    for k in O.leaves:
        d = key_depth(k)
        if d > depth:
            count[k >> (3 * (d - depth))] = count.get(k >> (3 * (d - depth)), 0) + 1
    return max(sorted(count), key=lambda k: count[k])


def level_parents(S, T, depth):
    """The seed leaves of node depth `depth` of (sub)tree S in Leaf_iterator order: (keys, seed leaf indices)."""
    from hpmvs_amd.frontier import key_depth
    keys, rows, _, _ = S.leaf_table()
    sel = [i for i, k in enumerate(keys) if key_depth(int(k)) == depth and isinstance(rows[i], (int, np.integer))]
    return [int(keys[i]) for i in sel], [int(rows[i]) for i in sel]


def two_lowest_levels(S):
    from hpmvs_amd.frontier import key_depth
    return sorted({key_depth(k) for k in S.leaves})[:2]


def reference_run(oscene, R, T, root_depth, abs_int, cache, with_filter=False):
    """The sequential loop over the two lowest populated levels of the (sub)tree, from the maps the seed tree leaves behind.
    -> (per level dict(ref, width, rows / cells), pointer tree, OracleDepths, subtree root key)"""
    from hpmvs_amd import frontier
    from oracle import oracle as orc
    O = frontier.Octree.from_seed_tree(T)
    root = subtree_root(O, root_depth)
    S = O.subtree(root) if root != 1 else O
    TR = otr.tree_from_keys(S.root_center, S.root_width, S.branches, S.leaves)
    OD = orc.OracleDepths(oscene)
    for i in T.rows:
        OD.set_depths(fr.oracle_patch(R, int(i))[0])
    out = []
    for depth in two_lowest_levels(S):
        keys, leaves = level_parents(S, T, depth)
        width = S.cell(keys[0])[1]
        rec = dict(depth=depth, width=width, leaves=leaves)
        if with_filter:
            cells = [T.rows[T.cell_start[l]:T.cell_start[l + 1]] for l in leaves]
            rows = np.concatenate(cells)
            cs = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int32)
            dist, keep = fr.filter_cells(R.center[rows], R.normal[rows], cs)
            kept = rows[keep]
            losers = [(c, int(rows[r])) for c in range(len(cells)) for r in range(cs[c], cs[c + 1]) if r != keep[c]]
            rec.update(rows=rows, cs=cs, dist=dist, keep=keep, losers=len(losers))
            ref = otr.sequential_extend(oscene, OD, _patches(R, kept), width, TR, MARGIN, abs_int, events=_patches(R, [r for _, r in losers]),
                                        event_cell=[c for c, _ in losers], cache=cache, cache_keys=[int(r) for r in kept])
        else:
            kept = np.array([int(T.rows[T.cell_start[l]]) for l in leaves])
            ref = otr.sequential_extend(oscene, OD, _patches(R, kept), width, TR, MARGIN, abs_int, cache=cache, cache_keys=[int(r) for r in kept])
        rec.update(ref=ref, parents=kept)
        out.append(rec)
    return out, TR, OD, root


def grid_differences(oscene, R, T, rec, abs_int):
    """Candidates of the level whose fate under the grid-key loop (oracle.extend_round, occupancy = the grid cells of every seed
    patch) differs from the loop on the real tree, from the same maps."""
    from oracle import oracle as orc
    OD = orc.OracleDepths(oscene)
    for i in T.rows:
        OD.set_depths(fr.oracle_patch(R, int(i))[0])
    occ = {orc.cell_key(R.center[int(i)], rec["width"]) for i in T.rows}
    cand, _ = orc.extend_round(oscene, OD, _patches(R, rec["parents"]), float(rec["width"]), occ, MARGIN, abs_int, frozen_gates=False)
    st = np.array([cand[t].stage for t in range(6 * len(rec["parents"]))])
    tree_st = rec["ref"]["stage"]
    return int(((st == 0) != (tree_st == 0)).sum()), int((st != tree_st).sum())


def _setup(tag):
    """scene, GPU scene, oracle scene and the refined survivors of a case, once per module"""
    if tag not in _state:
        from hpmvs_amd import api, synth
        from oracle import oracle as orc
        c = CASES[tag]
        scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
        g = api.Scene(scene, device=0)
        b = make_seed_batch(scene, c["groups"])
        api.optimize_batch(g, b)
        k = np.nonzero(b.ok)[0]
        R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
        R.ok[:] = 1
        orc.build()
        _state[tag] = dict(scene=scene, g=g, o=orc.OracleScene(scene), R=R, cache={})
    return _state[tag]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _state.values():
        s["g"].close()
    _state.clear()


def _maps_equal(g, OD):
    from hpmvs_amd import api
    for v in range(g.n_views):
        for l in range(g.view_levels[v]):
            a, b = api.depth_level(g, v, l), OD.level(v, l)
            if not np.array_equal(a, b):
                return (v, l, int((a != b).sum()))
    return None


def _run_case(tag, whole, abs_int, with_filter=False):
    from hpmvs_amd import api, frontier
    st = _setup(tag)
    g, R = st["g"], st["R"]
    c = CASES[tag]
    api.depth_reset(g)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=True)     # (floors R.scale in place: idempotent)
    ref_levels, TR, OD, root = reference_run(st["o"], R, T, 0 if whole else c["sub_depth"], abs_int, st["cache"], with_filter)
    O = frontier.Octree.from_seed_tree(T)
    S = O.subtree(root) if root != 1 else O
    assert len(ref_levels) == 2
    summary = []
    for rec in ref_levels:
        keys, leaves = level_parents(S, T, rec["depth"])
        assert leaves == rec["leaves"]
        ref = rec["ref"]
        if with_filter:
            P = frontier._rows(R, rec["rows"])
            F, L = frontier.filter_extend_level_tree(g, P, rec["cs"], rec["width"], S, margin=MARGIN, abs_int=abs_int)
            assert np.array_equal(F.keep, rec["keep"]) and F.dist.tobytes() == rec["dist"].tobytes()
        else:
            L = frontier.extend_level_tree(g, frontier._rows(R, rec["parents"]), rec["width"], S, MARGIN, abs_int)
        what = (tag, whole, abs_int, rec["depth"])
        diff = np.nonzero(L.stage != ref["stage"])[0]
        assert len(diff) == 0, (what, diff[:10], L.stage[diff[:10]], ref["stage"][diff[:10]])
        assert np.array_equal(L.counts, ref["counts"]), (what, np.nonzero((L.counts != ref["counts"]).any(axis=1))[0][:10])
        assert L.accepted == ref["accepted"] and L.border == ref["border"], what
        for t in np.nonzero(np.isin(ref["stage"], (0, 21, 22, 23, 24, 25, 26, 27)))[0]:
            assert np.array_equal(ref["center"][t], L.candidates.center[t]) and np.array_equal(ref["normal"][t], L.candidates.normal[t]), (what, t)
        summary.append(dict(depth=rec["depth"], parents=len(rec["parents"]), accepted=len(L.accepted), border=len(L.border), waves=L.waves,
                            losers=rec.get("losers", 0), tally={k: int(v) for k, v in ref["tally"].items()}))
    branches, leaves, _ = TR.key_sets()
    assert S.branches == branches and set(S.leaves) == set(leaves), (tag, whole, abs_int)
    bad = _maps_equal(g, OD)
    assert bad is None, (tag, whole, abs_int, bad)
    print("extend_level_tree", tag, "whole" if whole else f"subtree {root:#o}", "abs_int", abs_int, "filter" if with_filter else "", summary)
    return st, T, ref_levels


@pytest.mark.parametrize("abs_int", [0, 1])
@pytest.mark.parametrize("whole", [True, False], ids=["whole", "subtree"])
@pytest.mark.parametrize("tag", list(CASES))
def test_extend_level_tree_equals_the_sequential_loop(tag, whole, abs_int):
    _run_case(tag, whole, abs_int)


def test_filter_extend_level_tree_equals_the_sequential_loop():
    st, T, ref_levels = _run_case("configs0", True, 0, with_filter=True)
    assert sum(rec["losers"] for rec in ref_levels) >= 5          # the losers are there as events


def test_reference_loop_shows_every_case():
    """The six conditions on the CPU reference loop alone, over the cases above (abs_int 0)."""
    from hpmvs_amd import api, frontier
    total = {}
    for tag in CASES:
        st = _setup(tag)
        api.depth_reset(st["g"])
        T = frontier.seed_tree(st["g"], st["R"], patch_init_maxlevel=CASES[tag]["maxlevel"], set_depths=False)
        for whole in (True, False):
            ref_levels, _, _, _ = reference_run(st["o"], st["R"], T, 0 if whole else CASES[tag]["sub_depth"], 0, st["cache"])
            for rec in ref_levels:
                for k, v in rec["ref"]["tally"].items():
                    total[k] = total.get(k, 0) + int(v)
                if whole:
                    fate, stage = grid_differences(st["o"], st["R"], T, rec, 0)
                    total["grid_fate_differs"] = total.get("grid_fate_differs", 0) + fate
                    total["grid_stage_differs"] = total.get("grid_stage_differs", 0) + stage
    print("extend_level_tree reference tallies", total)
    for k in ("pre_shallower_nonempty", "pre_finer", "refused", "border", "deep_split", "grid_fate_differs"):
        assert total.get(k, 0) >= 1, (k, total)
