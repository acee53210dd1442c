"""frontier.process_level_forest -- ONE hpmvs_process_forest_batch for the regularize / settle sweep of all subtrees -- against
(a) the per-tree loop: frontier.process_level on tree 0, then tree 1, and so on, from the same starting maps, byte for byte;
(b) on configs[0], the TRUE sequential loop: orc.branch_round per leaf, OracleDepths.set_depths(p, subtract=True) for removals
    and tests/octree_ref.py's regularize on the pointer trees as they stand;
(c) the device-pointer form of the call against the host-pointer form.
Scenes and seeds are those of tests/test_gpu_extend_level_tree.py plus off-surface outliers (copies of refined patches moved six
leaf widths along their normal: isolated leaves, flatness 2.5 / 2.6 from regularize).  The forests are frontier.partition(g, O,
min_trees=8, min_split_leaves=4) of each scene's seed tree; the cells are every nonempty leaf's first patch, in tree order;
flatness and final_level are drawn as tests/test_gpu_process_level.py draws them.

Conditions, asserted on the per-tree loop alone (test_the_per_tree_loop_shows_every_case) and printed: at least 3 trees hold cells;
removed, split and children are all > 0; regularize yields both a constant (2.5 / 2.6) and an RMS value; at least one regularized
cell in a tree that is not the first with cells gets a flatness that differs from the one against the tree at the sweep's start;
at least one depth-map cell is touched by setDepths calls of two different trees (api.depth_footprints_batch of the op rows:
test_setdepths_calls_of_two_trees_meet_in_a_map_cell, which also says why the draw's seed is what it is).
The number of splits with two children in one octant is printed, not asserted (tests/test_cpu_process_forest.py covers it)."""
import copy
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
import octree_ref as ot
from test_gpu_extend_level_tree import CASES, _setup, _state

pytestmark = pytest.mark.gpu
f32 = np.float32
K, MIN_SPLIT = 8, 4
SEED = 94     # of the draw below (outliers, flatness, final_level): see test_setdepths_calls_of_two_trees_meet_in_a_map_cell
RESULTS = (("support", np.int32, 1), ("removed", np.uint8, 1), ("split", np.uint8, 1), ("children", np.uint8, 4),
           ("child_key", np.uint64, 4), ("n_neighbours", np.int32, 1), ("neighbour_key", np.uint64, 24))
_started = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _state.values():
        s["g"].close()
    _state.clear()
    _started.clear()


def _maps(g):
    from hpmvs_amd import api
    return {(v, l): api.depth_get_level(g, v, l) for v in range(g.n_views) for l in range(g.view_levels[v])}


def _restore(g, maps):
    from hpmvs_amd import api
    for (v, l), m in maps.items():
        api.depth_set_level(g, v, l, m)


def _start(tag):
    """Once per scene: the refined seeds plus outliers, the seed tree, its partition, the cells of every tree and their drawn
    flatness / final_level, and the maps the seed tree leaves behind."""
    if tag in _started:
        s = _started[tag]
        _restore(s["g"], s["maps"])
        return s
    from hpmvs_amd import api, frontier
    st = _setup(tag)
    g, R0 = st["g"], st["R"]
    rng = np.random.default_rng(len(tag) + SEED)
    k_out = max(8, R0.n // 20)
    pick = rng.permutation(R0.n)[:k_out]
    nrm = R0.normal[pick, :3] / np.linalg.norm(R0.normal[pick, :3], axis=1, keepdims=True)
    oc = R0.center[pick].copy()
    oc[:, :3] += (nrm * (6.0 * R0.scale[pick, None] * 2.0 / 0.9)).astype(f32)
    R = api.Batch(np.concatenate([R0.center, oc]), np.concatenate([R0.normal, R0.normal[pick]]), np.concatenate([R0.scale, R0.scale[pick]]),
                  np.concatenate([R0.n_images, R0.n_images[pick]]), np.concatenate([R0.images, R0.images[pick]]))
    R.ok[:] = 1
    api.depth_reset(g)
    T = frontier.seed_tree(g, R, patch_init_maxlevel=CASES[tag]["maxlevel"], set_depths=True)
    O = frontier.Octree.from_seed_tree(T)
    P = frontier.partition(g, O, min_trees=K, min_split_leaves=MIN_SPLIT)
    ct, ck, rows = [], [], []
    for k, S in enumerate(P.trees):
        keys, leaf_rows, _, _ = S.leaf_table()
        for key, l in zip(keys, leaf_rows):
            ct.append(k); ck.append(int(key)); rows.append(int(T.rows[T.cell_start[l]]))
    n = len(ct)
    rows = np.array(rows)
    fl = np.where(rng.random(n) < 0.5, -1.0, 0.0).astype(f32)
    rem = rng.random(n) < 0.08
    fl[rem] = np.where(rng.random(int(rem.sum())) < 0.5, 2.5, 2.6).astype(f32)
    fl[rows >= R0.n] = -1.0                                             # the outliers are regularized
    final = (rng.random(n) < 0.3).astype(np.uint8)
    cells = frontier._rows(R, rows)
    cells.ok[:] = 1
    s = dict(g=g, o=st["o"], scene=st["scene"], R=R, T=T, P=P, cells=cells, rows=rows, ct=np.array(ct, np.int32), ck=np.array(ck, np.uint64),
             fl=fl, final=final, maps=_maps(g), center={(t, key): R.center[r, :3] for t, key, r in zip(ct, ck, rows)})
    _started[tag] = s
    return s


def _per_tree_loop(s):
    """frontier.process_level on tree 0, then tree 1, ... on copies of the trees -> the sweep's result over the concatenated queue,
    keys in place of snapshot indices, the trees afterwards, and the ordered op rows with their tree."""
    from hpmvs_amd import api, frontier
    g, cells, ct, ck = s["g"], s["cells"], s["ct"], s["ck"]
    trees = copy.deepcopy(s["P"].trees)
    n = len(ct)
    W = dict(flatness=s["fl"].copy(), n_neighbours=np.zeros(n, np.int32), neighbour_key=np.zeros((n, 24), np.uint64), support=np.zeros(n, np.int32),
             removed=np.zeros(n, np.uint8), split=np.zeros(n, np.uint8), children=np.zeros((n, 4), np.uint8), child_key=np.zeros((n, 4), np.uint64),
             cand={}, start_flatness=s["fl"].copy(), same_octant=0, op_tree=[], op_rows=[])
    for k, S in enumerate(trees):
        idx = np.nonzero(ct == k)[0]
        if not len(idx):
            continue
        keys = [int(x) for x in ck[idx]]                                 # leaf_table order: cell j owns snapshot leaf j
        assert keys == [int(x) for x in S.leaf_table()[0]]
        snap = S.snapshot(np.array([s["center"][(k, key)] for key in keys], f32))
        sub = frontier._rows(cells, idx)
        reg = np.nonzero(s["fl"][idx] < 0)[0]
        if len(reg):                                                     # against the tree at the sweep's start
            W["start_flatness"][idx[reg]] = frontier.regularize_level(g, frontier._rows(sub, reg), snap.cell_width[reg], reg.astype(np.int32),
                                                                      np.ones(len(reg), np.uint8), snap, s["fl"][idx[reg]])[0]
        r = frontier.process_level(g, sub, np.arange(len(idx)), s["fl"][idx], np.ones(len(idx), np.uint8), snap, s["final"][idx], neighbours=True)
        leaf_key = list(keys)                                            # snapshot index -> key, the born leaves appended as process_level does
        for j, i in enumerate(r.settled):
            if r.settle.split[j]:
                seen = []
                for kk in range(4):
                    o_ = int(r.settle.child_octant[j, kk])
                    if o_ >= 0 and o_ not in seen:
                        seen.append(o_)
                        leaf_key.append((keys[i] << 3) | o_)
                W["same_octant"] += len(seen) < int(r.settle.children[j].sum())
        assert len(leaf_key) == r.snapshot.n
        leaf_key = np.array(leaf_key + [0], np.uint64)                   # (-1 -> 0)
        W["flatness"][idx] = r.flatness
        W["n_neighbours"][idx] = r.n_neighbours
        W["neighbour_key"][idx] = leaf_key[r.neighbour_leaf]
        st = idx[r.settled]
        W["support"][st] = r.settle.support
        W["removed"][st] = r.settle.removed
        W["split"][st] = r.settle.split
        W["children"][st] = r.settle.children
        W["child_key"][st] = leaf_key[r.child_leaf]
        for j, i in enumerate(st):
            W["cand"][int(i)] = (r.settle.candidates, j)
        # the caller's part: the tree operations in queue order, and the op rows for the footprints
        for j, i in enumerate(r.settled):
            key = keys[i]
            if r.settle.removed[j]:
                S.remove(key)
            elif r.settle.split[j]:
                S.split(key)
                for kk in range(4):
                    ckey = int(leaf_key[r.child_leaf[j, kk]]) if r.child_leaf[j, kk] >= 0 else 0
                    if ckey and ckey not in S.leaves:
                        S.insert(ckey, ("branch", 4 * int(idx[i]) + kk))
            if r.settle.removed[j] or r.settle.split[j]:
                W["op_tree"].append(k); W["op_rows"].append(("cell", int(idx[i])))
                for kk in np.nonzero(r.settle.children[j])[0] if r.settle.split[j] else []:
                    W["op_tree"].append(k); W["op_rows"].append(("child", r.settle.candidates, 4 * j + int(kk)))
    # support of the regularized cells: the call returns it for every row
    W["support"] = api.level_support_batch(g, cells, int(api.default_options().MINLEVEL))
    W["trees"] = trees
    return W


def _forest(s):
    from hpmvs_amd import frontier
    trees = copy.deepcopy(s["P"].trees)
    r = frontier.process_level_forest(s["g"], s["cells"], s["ct"], s["ck"], s["fl"], trees, s["center"], final_level=s["final"], neighbours=True)
    return r, trees


def _both(tag):
    s = _start(tag)
    if "loop" not in s:
        s["loop"] = _per_tree_loop(s)
        s["loop_maps"] = _maps(s["g"])
        _restore(s["g"], s["maps"])
        s["forest"], s["forest_trees"] = _forest(s)
        s["forest_maps"] = _maps(s["g"])
    return s


@pytest.mark.parametrize("tag", list(CASES))
def test_forest_sweep_equals_the_per_tree_loop(tag):
    from hpmvs_amd import api
    s = _both(tag)
    W, r = s["loop"], s["forest"]
    assert r.flatness.view(np.int32).tobytes() == W["flatness"].view(np.int32).tobytes(), np.nonzero(r.flatness != W["flatness"])[0][:10]
    for name in ("n_neighbours", "neighbour_key", "support", "removed", "split", "child_key"):
        assert getattr(r, name).tobytes() == W[name].tobytes(), (tag, name, np.nonzero(np.atleast_1d(getattr(r, name) != W[name]))[0][:10])
    assert r.children.astype(np.uint8).tobytes() == W["children"].tobytes(), tag
    for i, (cand, j) in W["cand"].items():                              # every field of the settled cells' candidates
        for name in api.Batch.FIELDS:
            assert getattr(r.candidates, name)[4 * i:4 * i + 4].tobytes() == getattr(cand, name)[4 * j:4 * j + 4].tobytes(), (tag, i, name)
    for k, (a, b) in enumerate(zip(s["forest_trees"], W["trees"])):
        assert a.branches == b.branches and a.leaves == b.leaves, (tag, k)
    for key, m in s["loop_maps"].items():
        assert np.array_equal(m, s["forest_maps"][key]), (tag, key, int((m != s["forest_maps"][key]).sum()))
    changed = sum(int((m != s["maps"][key]).sum()) for key, m in s["loop_maps"].items())
    print("process_level_forest", tag, dict(cells=len(s["ct"]), settled=len(W["cand"]), map_cells_changed=changed))
    assert changed > 0


def _shared_map_cells(s, W):
    """The depth-map cells the sweep's setDepths calls offer a depth to (api.depth_footprints_batch of the op rows) -> (calls,
    cells that two calls reach, cells that calls of two different trees reach)."""
    from hpmvs_amd import api
    rows = []
    for op in W["op_rows"]:
        src, t = (s["cells"], op[1]) if op[0] == "cell" else (op[1], op[2])
        rows.append((src.center[t], src.normal[t], src.scale[t], src.n_images[t], src.images[t]))
    ops = api.Batch(*[np.array([x[f] for x in rows]) for f in range(5)])
    wr = api.depth_footprints_batch(s["g"], ops)[0]
    owner, two_calls, two_trees = {}, 0, 0
    for j, (t, w) in enumerate(zip(W["op_tree"], wr)):
        for view, level, x, y in w[w[:, 0] >= 0]:
            prev = owner.setdefault((int(view), int(level), int(x), int(y)), (j, t))
            two_calls += prev[0] != j
            two_trees += prev[1] != t
    return len(rows), two_calls, two_trees


def _conditions():
    """Per scene, on the per-tree loop alone: the figures the two tests below assert on."""
    from hpmvs_amd import api
    out = {}
    for tag in CASES:
        s = _both(tag)
        W, ct, fl = s["loop"], s["ct"], s["fl"]
        reg = fl < 0
        const = np.isin(W["flatness"][reg], [f32(2.5), f32(2.6)])
        first = int(ct[0])
        versioned = reg & (ct != first) & (W["flatness"].view(np.int32) != W["start_flatness"].view(np.int32))
        n_calls, two_calls, two_trees = _shared_map_cells(s, W)
        out[tag] = dict(trees_with_cells=len(np.unique(ct)), removed=int(W["removed"].sum()), split=int(W["split"].sum()),
                        children=int(W["children"].sum()), constants=int(const.sum()), rms=int((~const).sum()), versioned=int(versioned.sum()),
                        setdepths_calls=n_calls, map_cells_of_two_calls=int(two_calls), map_cells_of_two_trees=int(two_trees),
                        splits_with_two_children_in_one_octant=int(W["same_octant"]))
        print("process_level_forest conditions", tag, out[tag])
    return out


def test_the_per_tree_loop_shows_every_case():
    """Every scene's figures are printed.  Every scene has cells in at least 3 trees; the other conditions hold for the two scenes
    taken together, as the conditions of tests/test_gpu_extend_level_forest.py do (configs[0] alone -- 3 views, 500 seeds -- is
    too sparse for regularize to find four neighbours: 142 constants, no RMS value; the 12-view scene has 260 and 23)."""
    per_scene = _conditions()
    total = {}
    for rep in per_scene.values():
        assert rep["trees_with_cells"] >= 3
        for k, v in rep.items():
            total[k] = total.get(k, 0) + v
    print("process_level_forest conditions, both scenes", total)
    for k in ("removed", "split", "children", "constants", "rms", "versioned"):
        assert total[k] > 0, (k, total)


def test_setdepths_calls_of_two_trees_meet_in_a_map_cell():
    """At least one depth-map cell is touched by setDepths calls of two different trees, over the two scenes.  The 12-view
    scene shows it (2 cells, 481 calls); configs[0] does NOT (238 calls; two calls of ONE tree meet on 41 cells there, a split
    leaf's patch and its children, never calls of two trees) and is reported here rather than asserted on its own.
    The subtrees are disjoint octants of one smooth surface, so first patches of two trees offer a depth to the same map cell
    only rarely (at most 29 pairs per scene over the seeds below), and almost every such pair has an off-surface outlier in it,
    which is regularized and makes no setDepths call.  The condition therefore hangs on the draw of outliers, flatness and
    final_level.  Seeds 90 .. 97 of that draw were run through the per-tree loop alone -- the code the parent commit has, not
    the forest call -- and 94 is the one among them whose loop shows every condition of this file; with the other seven no
    scene has such a cell.  test_twin_trees_share_every_map_cell exercises the same thing on a forest built for it."""
    per_scene = _conditions()
    assert sum(rep["map_cells_of_two_trees"] for rep in per_scene.values()) > 0, per_scene


def test_twin_trees_share_every_map_cell():
    """The subtree of configs[0] with the most cells, twice in one forest, each copy with all of its cells: every setDepths call
    of the second tree reaches map cells the first tree's calls reached before, so the order of the ONE replay across trees
    decides the maps.  The forest call equals the per-tree loop on the first copy, then the second, from the same maps."""
    from types import SimpleNamespace
    s = _both("configs0")
    k = int(np.bincount(s["ct"]).argmax())
    idx = np.nonzero(s["ct"] == k)[0]
    m = len(idx)
    twice = np.concatenate([idx, idx])
    from hpmvs_amd import frontier
    t = dict(s)
    t.update(P=SimpleNamespace(trees=[copy.deepcopy(s["P"].trees[k]), copy.deepcopy(s["P"].trees[k])]), cells=frontier._rows(s["cells"], twice),
             ct=np.repeat(np.arange(2, dtype=np.int32), m), ck=s["ck"][twice], fl=s["fl"][twice], final=s["final"][twice],
             center={(c, int(key)): s["center"][(k, int(key))] for c in (0, 1) for key in s["ck"][idx]})
    _restore(s["g"], s["maps"])
    W = _per_tree_loop(t)
    want = _maps(s["g"])
    _restore(s["g"], s["maps"])
    r, trees = _forest(t)
    got = _maps(s["g"])
    assert r.flatness.view(np.int32).tobytes() == W["flatness"].view(np.int32).tobytes()
    for name in ("n_neighbours", "neighbour_key", "support", "removed", "split", "child_key"):
        assert getattr(r, name).tobytes() == W[name].tobytes(), name
    assert r.children.astype(np.uint8).tobytes() == W["children"].tobytes()
    for a, b in zip(trees, W["trees"]):
        assert a.branches == b.branches and a.leaves == b.leaves
    for key, mm in want.items():
        assert np.array_equal(mm, got[key]), (key, int((mm != got[key]).sum()))
    n_calls, two_calls, two_trees = _shared_map_cells(t, W)
    print("process_level_forest twins", dict(cells=2 * m, setdepths_calls=n_calls, map_cells_of_two_trees=two_trees))
    assert two_trees > 0 and W["removed"][m:].tobytes() == W["removed"][:m].tobytes()
    _restore(s["g"], s["maps"])


# ---- (b) the true sequential loop

def _pointer_tree(S, P):
    """tests/octree_ref.py's pointer tree of an Octree whose rows index P."""
    t = ot.OctTree(S.root_center, S.root_width, P)

    def node(key):
        d = (int(key).bit_length() - 1) // 3
        n = t.root
        for lvl in range(d):
            if n.children is None:
                n.make_branch()
            n = n.children[(int(key) >> (3 * (d - 1 - lvl))) & 7]
        return n

    for k in S.branches:
        n = node(k)
        if n.children is None:
            n.make_branch()
    return t, node


def _keys_of(t):
    branches, leaves = set(), set()

    def key(n):
        path = []
        while n is not t.root:
            path.append(n.idx); n = n.parent
        k = 1
        for idx in reversed(path):
            k = (k << 3) | idx
        return k

    def walk(n):
        if n.children is None:
            if n.data:
                leaves.add(key(n))
            return
        if n is not t.root:
            branches.add(key(n))
        for ch in n.children:
            walk(ch)

    walk(t.root)
    return branches, leaves


def test_forest_sweep_equals_the_true_sequential_loop():
    from hpmvs_amd import api
    from oracle import oracle as orc
    tag = "configs0"
    s = _both(tag)
    r, scene, oscene, cells, ct, ck, fl = s["forest"], s["scene"], s["o"], s["cells"], s["ct"], s["ck"], s["fl"]
    n = len(ct)
    xax = [np.array(api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, 5).xaxis[:], f32) for v in scene.views]
    OD = orc.OracleDepths(oscene)
    for i in s["T"].rows:
        OD.set_depths(fr.oracle_patch(s["R"], int(i))[0])
    P = [c for c in cells.center[:, :3]]                                # element i: cell i's patch; the children are appended
    PT = []
    for k, S in enumerate(s["P"].trees):
        t, node = _pointer_tree(S, P)
        PT.append((t, node))
    leaf = []
    for i in range(n):
        t, node = PT[ct[i]]
        l = node(int(ck[i]))
        l.data.append(i)
        leaf.append(l)
    fl_seq, removed, split, children = fl.copy(), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8)
    for q in range(n):
        t = PT[ct[q]][0]
        if fl[q] < 0:
            fl_seq[q] = ot.regularize(t, cells.center[q], cells.normal[q], xax[int(cells.images[q, 0])], leaf[q].w, True, fl[q])[0]
        elif float(fl[q]) > 2.4:
            OD.set_depths(fr.oracle_patch(cells, q)[0], subtract=True)
            t.remove(leaf[q])
            removed[q] = 1
        else:
            cand, sp = orc.branch_round(oscene, OD, fr.oracle_patch(cells, q), leaf[q].c[None], np.array([leaf[q].w], f32), s["final"][q:q + 1],
                                        which=orc.OPT_REF)
            if sp[0]:
                split[q] = 1
                t.split(leaf[q])
                for k in range(4):
                    if cand[k].stage == 0:
                        children[q, k] = 1
                        c = np.array(cand[k].center[:3], dtype=f32)
                        P.append(c)
                        t.at(c, leaf[q]).data.append(len(P) - 1)
    assert r.flatness.view(np.int32).tobytes() == fl_seq.view(np.int32).tobytes(), np.nonzero(r.flatness != fl_seq)[0][:10]
    assert np.array_equal(r.removed, removed) and np.array_equal(r.split, split) and np.array_equal(r.children.astype(np.uint8), children)
    for k, S in enumerate(s["forest_trees"]):
        branches, leaves = _keys_of(PT[k][0])
        assert S.branches == branches and set(S.leaves) == leaves, k
    for (v, l), m in s["forest_maps"].items():
        assert np.array_equal(m, OD.level(v, l)), (v, l)


# ---- (c) the two pointer forms, and the refusals, through the C entry point

def _flat(s):
    from hpmvs_amd import frontier
    roots, bf, lf, bk, lk = frontier._flatten_forest(s["P"].trees)
    pc = np.zeros((len(lk), 3), f32)
    for t in range(len(s["P"].trees)):
        for l in range(int(lf[t]), int(lf[t + 1])):
            pc[l] = s["center"][(t, int(lk[l]))]
    return dict(roots=roots, bf=bf, lf=lf, bk=bk, lk=lk, pc=pc)


def _poison(shape, dt, fill=0x5A):
    return np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()


def raw_call(g, device, F, cells, ct, ck, fl, final, out_n=None, out_m=None, null=(), fill=0x5A):
    """One hpmvs_process_forest_batch through api.lib() on outputs filled with `fill` -> (status, dict of outputs, message).
    fill 0 where the two pointer forms are compared whole: the call leaves the tail of an image list, and colour and ncc of a
    candidate that failed, as it finds them (a staged host array arrives cleared)."""
    from hpmvs_amd import api
    n, M = cells.n, cells.max_images
    N, Mo = (4 * n if out_n is None else out_n), (M if out_m is None else out_m)
    shapes = dict(center=((N, 4), f32), normal=((N, 4), f32), scale=((N,), f32), n_images=((N,), np.int32), images=((N, Mo), np.int32),
                  ok=((N,), np.uint8), color=((N, 3), f32), ncc=((N,), f32), fmin=((N,), np.float64), x=((N, 3), np.float64),
                  result=((N,), np.int32), nevals=((N,), np.int32), stage=((N,), np.int32), ngrabs=((N,), np.int32))
    host = {k: _poison(sh, dt, fill) for k, (sh, dt) in shapes.items()}
    for name, dt, w in RESULTS:
        host[name] = _poison((n, w) if w > 1 else (n,), dt, fill)
    host["flatness"] = np.array(fl, f32).copy()
    ins = dict(bk=F["bk"], lk=F["lk"], pc=F["pc"], ct=np.ascontiguousarray(ct, np.int32), ck=np.ascontiguousarray(ck, np.uint64),
               final=np.ascontiguousarray(final, np.uint8))
    keep = {}
    if device:
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
        keep = {k: up(a) for k, a in list(host.items()) + list(ins.items()) if a.size}
        keep.update({"cell_" + name: up(getattr(cells, name)) for name in api.Batch.FIELDS if getattr(cells, name).size})
        ptr = lambda k: keep[k].data_ptr() if k in keep else None
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device="cuda:0")
        sp = C.c_void_p(stream.cuda_stream)
        cb = api.PatchBatch()
        cb.n, cb.max_images = n, M
        for name in api.Batch.FIELDS:
            setattr(cb, name, ptr("cell_" + name))
    else:
        ptr = lambda k: (host[k] if k in host else ins[k]).ctypes.data
        sp = None
        cb = cells.c_struct()
    ob = api.PatchBatch()
    ob.n, ob.max_images = N, Mo
    for name in api.Batch.FIELDS:
        setattr(ob, name, ptr(name))
    rb = api.ProcessForestResultStruct()
    for name, _, _ in RESULTS:
        setattr(rb, name, None if name in null else ptr(name))
    f = api.OctreeForest()
    f.n_trees = len(F["roots"])
    f.root, f.branch_first, f.leaf_first = F["roots"].ctypes.data, F["bf"].ctypes.data, F["lf"].ctypes.data
    f.branch_key, f.leaf_key = ptr("bk"), ptr("lk")
    o = api.default_options()
    status = api.lib().hpmvs_process_forest_batch(g.h, C.byref(o), C.byref(f), ptr("pc"), C.byref(cb), ptr("ct"), ptr("ck"), ptr("flatness"),
                                                  ptr("final"), C.byref(ob), None if null == "all" else C.byref(rb), 1 if device else 0, sp)
    message = api.lib().hpmvs_last_error().decode()
    if device:
        stream.synchronize()
        for k in host:
            if k in keep:
                host[k] = keep[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape)
    return status, host, message


def test_device_pointer_form_equals_the_host_pointer_form():
    for tag in CASES:
        s = _both(tag)
        F = _flat(s)
        got = {}
        for device in (0, 1):
            _restore(s["g"], s["maps"])
            status, got[device], message = raw_call(s["g"], device, F, s["cells"], s["ct"], s["ck"], s["fl"], s["final"], fill=0)
            assert status == 0, (tag, device, message)
            maps = _maps(s["g"])
            for key, m in s["forest_maps"].items():
                assert np.array_equal(m, maps[key]), (tag, device, key)
        for k in got[0]:
            assert got[0][k].tobytes() == got[1][k].tobytes(), (tag, k)
        r = s["forest"]
        assert got[0]["flatness"].tobytes() == r.flatness.tobytes() and got[0]["child_key"].tobytes() == r.child_key.tobytes()
        # without a result struct, and with single outputs left out, the sweep is the same
        for null in ("all", ("support", "children", "neighbour_key")):
            _restore(s["g"], s["maps"])
            status, h, message = raw_call(s["g"], 1, F, s["cells"], s["ct"], s["ck"], s["fl"], s["final"], null=null)
            assert status == 0, message
            assert h["flatness"].tobytes() == got[0]["flatness"].tobytes() and h["center"].tobytes() == got[0]["center"].tobytes()
            assert h["ok"].tobytes() == got[0]["ok"].tobytes() and h["fmin"].tobytes() == got[0]["fmin"].tobytes()
            maps = _maps(s["g"])
            assert all(np.array_equal(m, maps[key]) for key, m in s["forest_maps"].items())
            if null != "all":
                assert h["removed"].tobytes() == got[0]["removed"].tobytes() and (h["support"].view(np.uint8) == 0x5A).all()


def _untouched(h, fl, g, maps):
    for k, a in h.items():
        if k == "flatness":
            assert a.tobytes() == np.asarray(fl, f32).tobytes()
        else:
            assert (a.view(np.uint8) == 0x5A).all(), k
    now = _maps(g)
    assert all(np.array_equal(m, now[key]) for key, m in maps.items())


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_refusals_write_nothing(device):
    from hpmvs_amd import api, frontier
    s = _both("configs0")
    g, cells, ct, ck, fl, final = s["g"], s["cells"], s["ct"], s["ck"], s["fl"], s["final"]
    F = _flat(s)
    n = len(ct)
    lo, hi = n // 3, 2 * n // 3
    _restore(g, s["maps"])

    def refused(what, F2=F, cells2=cells, ct2=ct, ck2=ck, fl2=fl, code=-2, **kw):
        status, h, message = raw_call(g, device, F2, cells2, ct2, ck2, fl2, final, **kw)
        assert status == code and what in message, (what, status, message)
        _untouched(h, fl2, g, s["maps"])

    bad = ct.copy(); bad[[lo, hi]] = len(s["P"].trees)
    refused(f"cell {lo}: cell_tree", ct2=bad)
    bad = ck.copy(); bad[lo] = (int(ck[lo]) << 3) | 1; bad[hi] = 0
    refused(f"cell {lo}: cell_key is no nonempty leaf", ck2=bad)
    same = np.nonzero(ct == ct[lo])[0]
    a, b, c = same[0], same[len(same) // 2], same[-1]
    bad = ck.copy(); bad[[b, c]] = ck[a]
    refused(f"cell {b}: its leaf belongs to an earlier cell", ck2=bad)
    im = copy.deepcopy(cells)
    f2 = fl.copy(); f2[[lo, hi]] = -1.0
    im.images[[lo, hi], 0] = g.n_views
    refused(f"cell {lo}: a regularized cell's reference image", cells2=im, fl2=f2)
    F2 = dict(F); F2["lk"] = F["lk"].copy()
    t = int(ct[hi])
    F2["lk"][F["lf"][t] + 1] = F2["lk"][F["lf"][t]]
    refused(f"tree {t}: a key occurs twice", F2=F2)
    F2 = dict(F); F2["lf"] = F["lf"].copy(); F2["lf"][2] = F2["lf"][1] - 1
    refused("tree 1: the key offsets", F2=F2)
    refused("out->n must be 4", out_n=4 * n - 1)
    refused("max_images mismatch", out_m=cells.max_images + 1)
    # a leaf at depth 21 that would go to branch: a one-leaf tree appended to the forest
    deep = frontier.Octree(np.zeros(3, f32), 8.0)
    deep.insert((1 << 63) | 0o1234567, 0)
    roots, bf, lf, bk, lk = frontier._flatten_forest(s["P"].trees + [deep])
    F3 = dict(roots=roots, bf=bf, lf=lf, bk=bk, lk=lk, pc=np.concatenate([F["pc"], np.zeros((1, 3), f32)]))
    c3 = frontier._rows(cells, list(range(n)) + [0])
    ct3, ck3 = np.append(ct, len(s["P"].trees)).astype(np.int32), np.append(ck, np.uint64((1 << 63) | 0o1234567))
    fl3 = np.append(fl, f32(0.0))
    status, h, message = raw_call(g, device, F3, c3, ct3, ck3, fl3, np.append(final, 0))
    assert status == -2 and f"cell {n}: a leaf at depth 21" in message, message
    _untouched(h, fl3, g, s["maps"])
    # 5 n * max_images >= 2^28, refused on the sizes alone
    big = api.Batch(np.zeros((1, 4), f32), np.zeros((1, 4), f32), np.zeros(1, f32), np.zeros(1, np.int32), np.zeros((1, cells.max_images), np.int32))
    big.n = (1 << 28) // (5 * cells.max_images) + 1
    status = api.lib().hpmvs_process_forest_batch(g.h, C.byref(api.default_options()), C.byref(api.OctreeForest()), None, C.byref(big.c_struct()), None,
                                                  None, None, None, C.byref(_sized(4 * big.n, cells.max_images)), None, 0, None)
    assert status == -2 and "2^28" in api.lib().hpmvs_last_error().decode()


def _sized(n, m):
    from hpmvs_amd import api
    b = api.PatchBatch()
    b.n, b.max_images = n, m
    return b


def test_a_scene_without_depth_maps_is_refused():
    from hpmvs_amd import api
    s = _both("configs0")
    fresh = api.Scene(s["scene"], device=0)
    try:
        status, h, message = raw_call(fresh, 0, _flat(s), s["cells"], s["ct"], s["ck"], s["fl"], s["final"])
        assert status == -3 and "hpmvs_scene_depth_reset" in message, (status, message)
        assert all((a.view(np.uint8) == 0x5A).all() for k, a in h.items() if k != "flatness")
    finally:
        fresh.close()


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_degenerate_sweeps_succeed(device):
    from hpmvs_amd import frontier
    s = _both("configs0")
    g, cells, ct, ck, final = s["g"], s["cells"], s["ct"], s["ck"], s["final"]
    F = _flat(s)
    n = len(ct)
    _restore(g, s["maps"])
    status, h, message = raw_call(g, device, F, frontier._rows(cells, []), ct[:0], ck[:0], np.zeros(0, f32), final[:0])
    assert status == 0, message
    now = _maps(g)
    assert all(np.array_equal(m, now[key]) for key, m in s["maps"].items())
    status, h, message = raw_call(g, device, F, cells, ct, ck, np.full(n, -1.0, f32), final)       # all regularized: no depth op
    assert status == 0, message
    assert (h["n_neighbours"] >= 0).all() and not h["removed"].any() and not h["split"].any() and not h["ok"].any() and (h["stage"] == 20).all()
    now = _maps(g)
    assert all(np.array_equal(m, now[key]) for key, m in s["maps"].items())
    # ... and every cell sees the starting tree: the flatness of the per-tree loop's start
    reg = s["fl"] < 0
    assert h["flatness"][reg].tobytes() == s["loop"]["start_flatness"][reg].tobytes()
    status, h, message = raw_call(g, device, F, cells, ct, ck, np.zeros(n, f32), final)            # all settled
    assert status == 0, message
    assert (h["n_neighbours"] == -2).all() and h["split"].sum() > 0 and not h["neighbour_key"].any() and (h["flatness"] == 0).all()
    _restore(g, s["maps"])
