"""api.extend_forest_batch / hpmvs_extend_forest_batch against hpmvs_extend_tree_batch tree by tree: for every tree k the parents
with parent_tree == k in their given order go through api.extend_tree_batch alone, and the rows are scattered back -- the forest
call must return those bytes in all 14 batch fields and 5 key arrays, with host pointers and with device pointers, on outputs
that are over-allocated and poisoned (Buffers of tests/test_gpu_extend_tree_batch.py).  Scenes, trees and levels are those of
tests/test_gpu_extend_level_tree.py.

  one tree        the 8 (scene, whole / subtree, level) cases as forests of one tree
  a partition     frontier.partition(g, O, min_trees=8, min_split_leaves=4) of each scene's seed tree, the parents of each of the
                  two lowest populated seed levels shuffled so that tree ids interleave.  Asserted from the per-tree calls alone: at least 3
                  trees contribute, and the union shows a skip by a nonempty leaf, a skip by finer structure, a centre outside
                  the root, a refined candidate addConditional refuses and a border candidate
  equal keys      tree A, tree B = A without one nonempty leaf that pre-gates a candidate, tree C = A again, the same parents
                  for all three: A's and B's skip bytes differ, A's and C's rows are equal, the forest equals all three
  empties         no tree and no parent; trees without parents; a keyless tree in the middle with and without parents; a tree
                  rooted below the level without parents
  NULL outputs    every key output is nullable, one at a time
  refusals        each names the tree (or the parent) and leaves the poisoned outputs untouched; NULL inputs among them"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_extend_level_tree import CASES, level_parents, make_seed_batch, subtree_root, two_lowest_levels
from test_gpu_extend_tree_batch import HPMVS_ERR_ARG, KEYS, Buffers, assert_equals_composition

pytestmark = pytest.mark.gpu
f32 = np.float32
PARTITION = dict(min_trees=8, min_split_leaves=4)


class Tree:
    """One tree of a forest as the call takes it, and the Octree it came from (None for a hand-made one)."""

    def __init__(self, root_center, root_width, bk, lk, octree=None):
        self.root = np.array([*root_center, root_width], f32)
        self.bk, self.lk = np.ascontiguousarray(bk, np.uint64).reshape(-1), np.ascontiguousarray(lk, np.uint64).reshape(-1)
        self.octree = octree

    @classmethod
    def of(cls, S):
        return cls(S.root_center, S.root_width, S.branch_keys(), S.leaf_table()[0], S)


def per_tree(g, trees, parents, parent_tree, width):
    """The reference: api.extend_tree_batch per tree, scattered back -> (want Batch, key dict, per-tree results {k: (rows, out, keys)})."""
    from hpmvs_amd import api, frontier
    N, M = 6 * parents.n, parents.max_images
    want = api.Batch(np.zeros((N, 4), f32), np.zeros((N, 4), f32), np.zeros(N, f32), np.zeros(N, np.int32), np.zeros((N, M), np.int32))
    wkeys = {name: np.zeros(N, dt) for name, dt in KEYS}
    alone = {}
    for k, t in enumerate(trees):
        idx = np.nonzero(np.asarray(parent_tree) == k)[0]
        if not len(idx):
            continue
        out, keys = api.extend_tree_batch(g, frontier._rows(parents, idx), width, t.root[:3], t.root[3], t.bk, t.lk)
        rows = (6 * idx[:, None] + np.arange(6)[None, :]).reshape(-1)
        for name in api.Batch.FIELDS:
            getattr(want, name)[rows] = getattr(out, name)
        for name, _ in KEYS:
            wkeys[name][rows] = getattr(keys, name)
        alone[k] = (rows, out, keys)
    return want, wkeys, alone


def forest_call(g, device, trees, parents, parent_tree, width, null=(), missing=(), bf=None, lf=None, n_struct=None):
    """One hpmvs_extend_forest_batch through api.lib() on poisoned, over-allocated outputs -> (status, Buffers, message).
    missing: names of input pointers handed over as NULL; bf / lf: offsets in place of the trees' own."""
    from hpmvs_amd import api
    T = len(trees)
    roots = np.ascontiguousarray(np.array([t.root for t in trees], f32).reshape(T, 4))
    bfirst = np.concatenate([[0], np.cumsum([len(t.bk) for t in trees])]).astype(np.int32) if bf is None else np.asarray(bf, np.int32)
    lfirst = np.concatenate([[0], np.cumsum([len(t.lk) for t in trees])]).astype(np.int32) if lf is None else np.asarray(lf, np.int32)
    bk = np.concatenate([t.bk for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    lk = np.concatenate([t.lk for t in trees] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    pt = np.ascontiguousarray(parent_tree, np.int32).reshape(-1)
    B = Buffers(6 * parents.n, parents.max_images, device, n_struct, null)
    keep = []
    if device:
        import torch
        up = lambda a: (keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")) or keep[-1].data_ptr()) if a.size else None
        pb = api.PatchBatch()
        pb.n, pb.max_images = parents.n, parents.max_images
        for name in api.Batch.FIELDS:
            setattr(pb, name, up(getattr(parents, name)))
        pbk, plk, ppt = up(bk), up(lk), up(pt)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device="cuda:0")
        sp = C.c_void_p(stream.cuda_stream)
    else:
        pb = parents.c_struct()
        pbk, plk, ppt = bk.ctypes.data, lk.ctypes.data, pt.ctypes.data
        sp = None
    f = api.OctreeForest()
    f.n_trees = T
    f.root = None if "root" in missing else roots.ctypes.data
    f.branch_first = None if "branch_first" in missing else bfirst.ctypes.data
    f.leaf_first = None if "leaf_first" in missing else lfirst.ctypes.data
    f.branch_key = None if "branch_key" in missing else pbk
    f.leaf_key = None if "leaf_key" in missing else plk
    o = api.default_options()
    status = api.lib().hpmvs_extend_forest_batch(g.h, C.byref(o), C.byref(f), C.byref(pb), None if "parent_tree" in missing else ppt,
                                                 float(width), C.byref(B.pb), C.byref(B.kb), 1 if device else 0, sp)
    message = api.lib().hpmvs_last_error().decode()
    if device:
        stream.synchronize()
    B.fetch()
    return status, B, message


@pytest.fixture(scope="module")
def scenes():
    """Per scene: the GPU scene, the refined seeds R, the seed tree T and its Octree O."""
    from hpmvs_amd import api, frontier, synth
    out = {}
    for tag, c in CASES.items():
        scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
        g = api.Scene(scene, device=0)
        b = make_seed_batch(scene, c["groups"])
        api.optimize_batch(g, b)
        k = np.nonzero(b.ok)[0]
        R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
        R.ok[:] = 1
        T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=False)
        out[tag] = dict(g=g, R=R, T=T, O=frontier.Octree.from_seed_tree(T), sub_depth=c["sub_depth"])
    yield out
    for s in out.values():
        s["g"].close()


def seed_parents(s, S, depth):
    """The parents of (sub)tree S on its depth `depth`: the first patch of every seed leaf there, and the level's width."""
    from hpmvs_amd import frontier
    keys, leaves = level_parents(S, s["T"], depth)
    return frontier._rows(s["R"], [int(s["T"].rows[s["T"].cell_start[l]]) for l in leaves]), (S.cell(keys[0])[1] if keys else None)


@pytest.fixture(scope="module")
def single(scenes):
    """The 8 (scene, whole / subtree, level) cases of tests/test_gpu_extend_tree_batch.py, each with its per-tree result."""
    out = []
    for tag, s in scenes.items():
        for whole in (True, False):
            root = subtree_root(s["O"], 0 if whole else s["sub_depth"])
            S = s["O"].subtree(root) if root != 1 else s["O"]
            for depth in two_lowest_levels(S):
                parents, width = seed_parents(s, S, depth)
                t = Tree.of(S)
                pt = np.zeros(parents.n, np.int32)
                want, wkeys, _ = per_tree(s["g"], [t], parents, pt, width)
                out.append(dict(what=(tag, "whole" if whole else "subtree", depth), g=s["g"], tree=t, parents=parents, pt=pt, width=f32(width),
                                want=want, keys=wkeys))
    return out


def partition_levels(s, shuffle_seed=5):
    """The subtrees of the scene's seed tree and, for each of its two lowest populated seed levels, the parents of all subtrees
    on that level, shuffled: [(depth, trees, parents, parent_tree, width)]."""
    from hpmvs_amd import frontier
    from hpmvs_amd.frontier import key_depth
    O = s["O"]
    P = frontier.partition(s["g"], O, **PARTITION)
    trees = [Tree.of(S) for S in P.trees]
    out = []
    for D in two_lowest_levels(O):
        width = O.cell(next(k for k in O.leaves if key_depth(k) == D))[1]
        rows, pt = [], []
        for k, S in enumerate(P.trees):
            d = D - key_depth(int(P.root_key[k]))
            if d < 1:
                continue
            _, leaves = level_parents(S, s["T"], d)
            rows += [int(s["T"].rows[s["T"].cell_start[l]]) for l in leaves]
            pt += [k] * len(leaves)
        order = np.random.default_rng(shuffle_seed).permutation(len(rows))
        out.append((D, trees, frontier._rows(s["R"], np.array(rows, np.int64)[order]), np.array(pt, np.int32)[order], f32(width)))
    return out


@pytest.fixture(scope="module")
def partitions(scenes):
    out = []
    for tag, s in scenes.items():
        for D, trees, parents, pt, width in partition_levels(s):
            want, wkeys, alone = per_tree(s["g"], trees, parents, pt, width)
            out.append(dict(what=(tag, "partition", D), g=s["g"], trees=trees, parents=parents, pt=pt, width=width, want=want, keys=wkeys, alone=alone))
    return out


def tally_alone(trees, alone, width):
    """What the per-tree calls show, from their own outputs and the host trees."""
    t = dict(skip_nonempty=0, skip_finer=0, outside_pre=0, refined_refused=0, refined_border=0)
    for k, (_, out, keys) in alone.items():
        S = trees[k].octree
        for c in np.nonzero(keys.skip)[0]:                 # a skipped candidate is built, not refined: its centre is the one looked up
            leaf = S.at(out.center[c])
            nonempty = leaf in S.leaves
            assert nonempty or S.cell(leaf)[1] < width
            t["skip_nonempty" if nonempty else "skip_finer"] += 1
        ok, border = out.ok != 0, keys.border != 0
        t["outside_pre"] += int((keys.pre_inside == 0).sum())
        t["refined_refused"] += int((ok & ~border & (keys.post_key == 0)).sum())
        t["refined_border"] += int(border.sum())
    return t


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_forest_of_one_tree_equals_extend_tree_batch(single, device):
    assert len(single) == 8
    for c in single:
        status, B, msg = forest_call(c["g"], device, [c["tree"]], c["parents"], c["pt"], c["width"])
        assert status == 0, (c["what"], msg)
        assert_equals_composition(B, c["want"], c["keys"], c["what"])


def test_the_partitions_show_every_case(partitions):
    total = {}
    for c in partitions:
        with_parents = sorted(c["alone"])
        t = tally_alone(c["trees"], c["alone"], c["width"])
        print("extend_forest_batch", c["what"], "trees", len(c["trees"]), "with parents", with_parents,
              "parents per tree", [int((c["pt"] == k).sum()) for k in with_parents], t)
        assert len(with_parents) >= 3, (c["what"], with_parents)
        assert (np.diff(c["pt"]) < 0).any(), "the tree ids do not interleave"
        for k, v in t.items():
            total[k] = total.get(k, 0) + v
    assert min(total.values()) >= 1, total


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_real_partition_equals_the_per_tree_calls(partitions, device):
    for c in partitions:
        status, B, msg = forest_call(c["g"], device, c["trees"], c["parents"], c["pt"], c["width"])
        assert status == 0, (c["what"], msg)
        assert_equals_composition(B, c["want"], c["keys"], c["what"])


def test_api_extend_forest_batch_equals_the_per_tree_calls(partitions):
    from hpmvs_amd import api
    c = partitions[0]
    tr = c["trees"]
    first = lambda a: np.concatenate([[0], np.cumsum([len(x) for x in a])])
    out, k = api.extend_forest_batch(c["g"], c["parents"], c["pt"], c["width"], [t.root for t in tr], first([t.bk for t in tr]),
                                     first([t.lk for t in tr]), np.concatenate([t.bk for t in tr]), np.concatenate([t.lk for t in tr]))
    for name in api.Batch.FIELDS:
        assert getattr(out, name).tobytes() == getattr(c["want"], name).tobytes(), name
    for name, _ in KEYS:
        assert getattr(k, name).tobytes() == c["keys"][name].tobytes(), name


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_null_key_outputs_one_at_a_time(partitions, device):
    c = min(partitions, key=lambda c: c["parents"].n)
    for name, _ in KEYS:
        status, B, msg = forest_call(c["g"], device, c["trees"], c["parents"], c["pt"], c["width"], null=(name,))
        assert status == 0, (name, msg)
        assert_equals_composition(B, c["want"], c["keys"], (c["what"], "without", name), null=(name,))


@pytest.fixture(scope="module")
def twins(single):
    """Tree A (the smallest subtree case), B = A without one nonempty leaf that pre-gates a candidate, C = A.  Every parent is
    given three times in a row, once per tree, so the tree ids interleave and each tree sees the parents in their own order."""
    from hpmvs_amd import frontier
    c = min((c for c in single if c["what"][1] == "subtree"), key=lambda c: c["parents"].n)
    A, S = c["tree"], c["tree"].octree
    gate = next(S.at(c["want"].center[t]) for t in np.nonzero(c["keys"]["skip"])[0] if S.at(c["want"].center[t]) in S.leaves)
    Bt = Tree(A.root[:3], A.root[3], A.bk, A.lk[A.lk != np.uint64(gate)])
    assert len(Bt.lk) == len(A.lk) - 1
    n = c["parents"].n
    parents = frontier._rows(c["parents"], np.repeat(np.arange(n), 3))
    pt = np.tile(np.arange(3, dtype=np.int32), n)
    trees = [A, Bt, A]
    want, wkeys, alone = per_tree(c["g"], trees, parents, pt, c["width"])
    return dict(what=("equal keys",) + c["what"], g=c["g"], trees=trees, parents=parents, pt=pt, width=c["width"], want=want, keys=wkeys, alone=alone)


def test_equal_keys_per_tree_results(twins):
    """The conditions of the equal-keys case, on the per-tree calls alone."""
    from hpmvs_amd import api
    (_, oa, ka), (_, ob, kb), (_, oc, kc) = (twins["alone"][k] for k in range(3))
    assert int((ka.skip != kb.skip).sum()) >= 1
    for name in api.Batch.FIELDS:
        assert getattr(oa, name).tobytes() == getattr(oc, name).tobytes(), name
    for name, _ in KEYS:
        assert getattr(ka, name).tobytes() == getattr(kc, name).tobytes(), name


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_equal_keys_in_different_trees_never_meet(twins, device):
    c = twins
    status, B, msg = forest_call(c["g"], device, c["trees"], c["parents"], c["pt"], c["width"])
    assert status == 0, msg
    assert_equals_composition(B, c["want"], c["keys"], c["what"])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_empties(partitions, device):
    from hpmvs_amd import frontier
    c = min(partitions, key=lambda c: c["parents"].n)
    g, none = c["g"], frontier._rows(c["parents"], [])
    # no tree, no parent
    status, B, msg = forest_call(g, device, [], none, [], c["width"])
    assert status == 0 and B.touched(whole=True) == [], msg
    # trees, no parent
    status, B, msg = forest_call(g, device, c["trees"], none, [], c["width"])
    assert status == 0 and B.touched(whole=True) == [], msg
    # a keyless tree in the middle (eight empty leaves under the root of tree 0), with and without parents; behind it a tree
    # rooted BELOW the level (its root is as wide as the level's leaves), without parents
    k0 = min(c["alone"])
    t0 = c["trees"][k0]
    keyless = Tree(t0.root[:3], t0.root[3], [], [])
    below = Tree(t0.root[:3], c["width"], [], c["trees"][k0].lk[:0])
    trees = [t0, keyless, t0, below]
    idx = np.nonzero(c["pt"] == k0)[0]
    parents = frontier._rows(c["parents"], np.concatenate([idx, idx, idx]))
    for pt in (np.repeat([0, 1, 2], len(idx)), np.repeat([0, 2, 0], len(idx))):
        pt = pt.astype(np.int32)
        want, wkeys, alone = per_tree(g, trees, parents, pt, c["width"])
        if 1 in alone:
            assert alone[1][2].skip.sum() == 0 and alone[1][1].ok.any()      # nothing gates in a keyless tree
        status, B, msg = forest_call(g, device, trees, parents, pt, c["width"])
        assert status == 0, msg
        assert_equals_composition(B, want, wkeys, ("keyless tree", pt[len(idx)]))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_name_the_tree_and_write_nothing(partitions, device):
    c = min(partitions, key=lambda c: c["parents"].n)
    g, trees, parents, pt, width = c["g"], c["trees"], c["parents"], c["pt"], c["width"]
    T = len(trees)
    with_parents = sorted(c["alone"])
    mid = with_parents[len(with_parents) // 2]
    assert 0 < mid < T - 1 and parents.n >= 5 and len(trees[mid].bk) and len(trees[mid].lk)
    m = trees[mid]
    deepest = int(max(m.lk))
    assert deepest < (1 << 57)
    swap = lambda t: trees[:mid] + [t] + trees[mid + 1:]
    narrow = Tree(m.root[:3], width, m.bk, m.lk)                       # its root is a leaf of the level: no level below it
    bf = np.concatenate([[0], np.cumsum([len(t.bk) for t in trees])]).astype(np.int32)
    lf = np.concatenate([[0], np.cumsum([len(t.lk) for t in trees])]).astype(np.int32)
    bf_bad, lf_bad = bf.copy(), lf.copy()
    bf_bad[mid + 1] = bf_bad[mid] - 1
    lf_bad[mid + 1] = lf_bad[mid] - 1
    first_bad = lf.copy()
    first_bad[0] = 1
    at = lambda v: np.concatenate([pt[:3], [v], pt[4:]]).astype(np.int32)
    bad_root = m.root.copy()
    bad_root[1] = np.nan
    tree_msg = f"tree {mid}:"
    refusals = {
        "a word that is no key": (dict(trees=swap(Tree(m.root[:3], m.root[3], m.bk, np.concatenate([m.lk, [np.uint64(2)]])))), tree_msg),
        "a doubled key": (dict(trees=swap(Tree(m.root[:3], m.root[3], m.bk, np.concatenate([m.lk, m.lk[:1]])))), tree_msg),
        "a key that is branch and leaf": (dict(trees=swap(Tree(m.root[:3], m.root[3], np.concatenate([m.bk, m.lk[:1]]), m.lk))), tree_msg),
        "an orphaned key": (dict(trees=swap(Tree(m.root[:3], m.root[3], m.bk, np.concatenate([m.lk, [np.uint64((deepest << 6) | 0o11)]])))), tree_msg),
        "branch offsets that decrease": (dict(bf=bf_bad), tree_msg),
        "leaf offsets that decrease": (dict(lf=lf_bad), tree_msg),
        "offsets that do not start at 0": (dict(lf=first_bad), "tree 0:"),
        "parent_tree of -1": (dict(parent_tree=at(-1)), "parent_tree[3]"),
        "parent_tree of n_trees": (dict(parent_tree=at(T)), "parent_tree[3]"),
        "a parent in a tree rooted below the level": (dict(trees=swap(narrow)), tree_msg),
        "a root that is not finite": (dict(trees=swap(Tree(bad_root[:3], bad_root[3], m.bk, m.lk))), tree_msg),
        "a root without width": (dict(trees=swap(Tree(m.root[:3], 0.0, m.bk, m.lk))), tree_msg),
        "NaN width": (dict(width=f32(np.nan)), ""),
        "out->n != 6 n": (dict(n_struct=6 * parents.n - 1), ""),
        "NULL root": (dict(missing=("root",)), ""),
        "NULL branch_first": (dict(missing=("branch_first",)), ""),
        "NULL leaf_first": (dict(missing=("leaf_first",)), ""),
        "NULL branch_key": (dict(missing=("branch_key",)), ""),
        "NULL leaf_key": (dict(missing=("leaf_key",)), ""),
        "NULL parent_tree": (dict(missing=("parent_tree",)), ""),
    }
    for what, (kw, names) in refusals.items():
        kw = dict(dict(trees=trees, parent_tree=pt, width=width), **kw)
        status, B, msg = forest_call(g, device, kw.pop("trees"), parents, kw.pop("parent_tree"), kw.pop("width"), **kw)
        assert status == HPMVS_ERR_ARG, (what, status, msg)
        assert names in msg, (what, msg)
        assert B.touched(whole=True) == [], (what, B.touched(whole=True))
