"""CellProcessor::regularize (reference src/hpmvs/CellProcessor.cpp:309-367) on the GPU: hpmvs_regularize_batch /
hpmvs_amd.frontier.regularize_level against the float32 restatement of DynOctTree and regularize in tests/octree_ref.py, bit for
bit -- flatness, neighbour count and the set of neighbour leaves -- on trees built with DynOctTree::add(p, width) from refined
seeds, on subtrees, and on versioned (born / died) tables where every cell must see the tree as it stands at its queue position."""
import numpy as np
import pytest

import octree_ref as ot

pytestmark = pytest.mark.gpu

# The kernel sums the squared plane distances in first-probe order, the reference in std::set<Leaf*> (heap-address) order: at most
# 23 float additions of non-negative terms round differently, so the two flatness values differ by less than 2^-19 relative
# (DESIGN.md §3.8).
ORDER_BOUND = 2.0 ** -19


def _refined(scene, gscene, n, seed_off):
    from hpmvs_amd import api, synth
    seeds = synth.make_seeds(scene, n, start_level=2, seed=synth.SEED + seed_off)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gscene, b)
    keep = np.nonzero(b.ok)[0]
    assert len(keep) > n // 2
    return api.Batch(b.center[keep], b.normal[keep], b.scale[keep], b.n_images[keep], b.images[keep])


def _xaxes(scene):
    from hpmvs_amd import api
    return [np.array(api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, 5).xaxis[:], np.float32) for v in scene.views]


def _build(R, rng, dup=0.1):
    """A DynOctTree over the refined patches, leaves on three or more depths; and leaves chosen to receive a second element."""
    P = R.center[:, :3].astype(np.float32)
    lo, hi = P.min(axis=0), P.max(axis=0)
    rc = ((lo + hi) / 2).astype(np.float32)
    rw = np.float32(2.0 ** np.ceil(np.log2(float((hi - lo).max()) * 1.1)))
    tree = ot.OctTree(rc, rw, P)
    base = (R.scale * np.float32(2.0 / 0.9)).astype(np.float32)
    width = (base * np.exp2(rng.integers(0, 4, size=R.n))).astype(np.float32)
    order = rng.permutation(R.n)
    for e in order:
        tree.add(int(e), width[e])
    # a few more elements into leaves that already hold one (a copy of a patch nudged inside its leaf: data[1])
    extra = []
    for e in order[: int(dup * R.n)]:
        leaf = tree.at(P[e])
        extra.append((leaf, int(e)))
    return tree, extra


def _table(tree, leaves, born=None, died=None):
    from hpmvs_amd import frontier
    return frontier.OctreeSnapshot(tree.root.c, tree.root.w, np.array([l.c for l in leaves]), np.array([l.w for l in leaves]),
                                   np.array([tree.P[l.data[0]] for l in leaves]), born, died)


def _compare(tag, gscene, tree, R, xax, cells, cell_leaf, expanded, flat_in, snap, position, trees_at=None, stats=None):
    from hpmvs_amd import api, frontier
    idx = np.array(cells)
    sub = api.Batch(R.center[idx], R.normal[idx], R.scale[idx], R.n_images[idx], R.images[idx])
    cw = np.array([cell_leaf[i].w for i in cells], np.float32)
    fl, nn, nb = frontier.regularize_level(gscene, sub, cw, position, expanded, snap, flat_in, neighbours=True)
    index = {(snap.cell_center[j].tobytes(), snap.cell_width[j].tobytes()): j for j in range(snap.n)}   # unique in these tables
    key = lambda l: (np.asarray(l.c, np.float32).tobytes(), np.float32(l.w).tobytes())
    for j, i in enumerate(cells):
        tr = tree if trees_at is None else trees_at(int(position[j]))
        want, found = ot.regularize(tr, R.center[i], R.normal[i], xax[int(R.images[i, 0])], cw[j], expanded[j], flat_in[j])
        got = fl[j]
        assert got.tobytes() == np.float32(want).tobytes(), (tag, j, got, want)
        if not expanded[j]:
            assert nn[j] == -1 and (nb[j] == -1).all()
            if stats is not None:
                stats["untouched"] += 1
            continue
        assert nn[j] == len(found), (tag, j, nn[j], len(found))
        assert list(nb[j, : nn[j]]) == [index[key(l)] for l in found], (tag, j)
        assert (nb[j, nn[j]:] == -1).all()
        if stats is None:
            continue
        stats["k0"] += len(found) == 0
        stats["k1_3"] += 1 <= len(found) < 4
        stats["own_leaf"] += any(l is cell_leaf[i] for l in found)
        stats["two_patches"] += any(len(l.data) > 1 for l in found)
        half = float(tr.root.w) / 2
        stats["outside_root"] += sum(any(abs(float(p[k]) - float(tr.root.c[k])) > half for k in range(3))
                                     for p in ot.probes(R.center[i], R.normal[i], xax[int(R.images[i, 0])], cw[j]))
        if len(found) >= 4:
            k = len(found)
            for order in (list(range(k))[::-1], list(np.random.default_rng(j).permutation(k))):
                alt, _ = ot.regularize(tr, R.center[i], R.normal[i], xax[int(R.images[i, 0])], cw[j], True, -1.0, order=order)
                d = abs(float(alt) - float(got))
                assert d <= ORDER_BOUND * float(got), (tag, j, float(alt), float(got))
                stats["max_order_rel"] = max(stats["max_order_rel"], d / float(got) if got else 0.0)
    return fl, nn


def _scene_case(tag, scene, gscene, n_seeds, seed_off):
    from hpmvs_amd import api
    rng = np.random.default_rng(seed_off)
    R0 = _refined(scene, gscene, n_seeds, seed_off)
    n0 = R0.n
    xax = _xaxes(scene)
    # off-surface outliers (inserted: their probes find little but their own leaf) and ghosts (cells whose patch is in no leaf)
    nrm = R0.normal[:, :3] / np.linalg.norm(R0.normal[:, :3], axis=1, keepdims=True)
    width0 = (R0.scale * np.float32(2.0 / 0.9)).astype(np.float32)
    span = float(np.ptp(R0.center[:, :3], axis=0).max())
    k_out = max(8, n0 // 20)
    pick = rng.permutation(n0)[: 2 * k_out]
    c_out = R0.center[pick].copy()
    c_out[:k_out, :3] += (nrm[pick[:k_out]] * (8.0 * width0[pick[:k_out], None])).astype(np.float32)
    c_out[k_out:, :3] += (nrm[pick[k_out:]] * (0.3 * span)).astype(np.float32)
    R = api.Batch(np.concatenate([R0.center, c_out]), np.concatenate([R0.normal, R0.normal[pick]]), np.concatenate([R0.scale, R0.scale[pick]]),
                  np.concatenate([R0.n_images, R0.n_images[pick]]), np.concatenate([R0.images, R0.images[pick]]))
    tree, extra = _build(api.Batch(R.center[: n0 + k_out], R.normal[: n0 + k_out], R.scale[: n0 + k_out], R.n_images[: n0 + k_out],
                                   R.images[: n0 + k_out]), rng)
    tree.P = R.center[:, :3].astype(np.float32)
    # second elements of their leaves: a patch moved half way to its leaf's centre (still inside; data[0] stays the first).  The
    # snapshot carries data[0] only (the C ABI's contract), so these check that the table is built from data[0], not data[1].
    for leaf, e in extra:
        moved = (tree.P[e] + (np.asarray(leaf.c, np.float32) - tree.P[e]) * np.float32(0.5)).astype(np.float32)
        tree.P = np.concatenate([tree.P, moved[None]])
        leaf.data.append(len(tree.P) - 1)
    leaves = tree.nonempty()
    depths = {tree.depth(l) for l in leaves}
    assert len(depths) >= 3, depths
    cells = list(range(R.n))
    cell_leaf = {i: tree.at(tree.P[i]) for i in cells}
    expanded = (rng.random(R.n) < 0.85).astype(np.uint8)
    flat_in = np.where(rng.random(R.n) < 0.5, -1.0, 0.0).astype(np.float32)
    stats = dict(k0=0, k1_3=0, own_leaf=0, two_patches=0, outside_root=0, untouched=0, max_order_rel=0.0)
    snap = _table(tree, leaves)
    _compare(tag, gscene, tree, R, xax, cells, cell_leaf, expanded, flat_in, snap, np.zeros(R.n, np.int32), stats=stats)
    # a subtree root that is not the global root: the root's child branch with the most leaves
    br = max((ch for ch in tree.root.children if ch.children is not None), key=lambda ch: len(tree.nonempty(ch)))
    sub = ot.OctTree.__new__(ot.OctTree)
    sub.root, sub.P = br, tree.P
    sleaves = sub.nonempty()
    scells = [i for i in cells if any(cell_leaf[i] is l for l in sleaves)]
    sstats = dict(stats, outside_root=0)
    _compare(tag + "/subtree", gscene, sub, R, xax, scells, cell_leaf, expanded[scells], flat_in[scells], _table(sub, sleaves),
             np.zeros(len(scells), np.int32), stats=sstats)
    print(tag, stats, "subtree outside-root probes:", sstats["outside_root"], "depths:", sorted(depths))
    for k in ("k0", "k1_3", "own_leaf", "two_patches", "outside_root", "untouched"):
        assert stats[k] > 0, (tag, k)
    assert sstats["outside_root"] > 0


def test_regularize_equals_the_restatement_on_configs0(tiny_scene, gpu_scene):
    _scene_case("configs0_3v_640x480", tiny_scene, gpu_scene, 900, 41)


def test_regularize_equals_the_restatement_on_a_12_view_scene():
    from hpmvs_amd import api, synth
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        _scene_case("12v_640x480", scene, g, 1400, 43)
    finally:
        g.close()


def test_versioned_table_gives_the_tree_at_each_position(tiny_scene, gpu_scene):
    """Random removals and splits at queue positions 0, 2, 4, ...; cells regularized at the odd positions between them.  Each cell
    equals the restatement run on the tree as it stands at its turn, and some differ from the tree at the sweep's start."""
    from hpmvs_amd import api
    rng = np.random.default_rng(77)
    R = _refined(tiny_scene, gpu_scene, 900, 51)
    xax = _xaxes(tiny_scene)
    tree, _ = _build(R, rng, dup=0.0)
    leaves0 = tree.nonempty()
    L0 = len(leaves0)
    owner = {}
    for l in leaves0:
        for e in l.data:
            owner[e] = l
    # the operations: one per even position, each on a distinct original leaf
    n_ops = L0 // 3
    victims = rng.permutation(L0)[:n_ops]
    ops = []
    P_ext = list(tree.P)
    for s, v in enumerate(victims):
        leaf = leaves0[v]
        if rng.random() < 0.5:
            ops.append(("remove", 2 * s, v, None))
        else:   # split: 1..4 new elements placed inside the leaf, data[0] of each child leaf = the first that lands there
            pts = []
            for _ in range(int(rng.integers(1, 5))):
                off = (rng.random(3) - 0.5) * 0.98 * float(leaf.w)
                P_ext.append((leaf.c + off).astype(np.float32))
                pts.append(len(P_ext) - 1)
            ops.append(("split", 2 * s, v, pts))
    P_all = np.array(P_ext, np.float32)
    # the versioned table: originals, then the split children (in op order, octant order of first appearance)
    born = [-1] * L0
    died = [api.INT32_MAX] * L0
    cc, cwid, pc = [l.c for l in leaves0], [l.w for l in leaves0], [tree.P[l.data[0]] for l in leaves0]
    for kind, s, v, pts in ops:
        died[v] = s
        if kind == "split":
            par = leaves0[v]
            seen = {}
            for e in pts:
                p = P_all[e]
                idx = (int(p[2] > par.c[2]) << 2) | (int(p[1] > par.c[1]) << 1) | int(p[0] > par.c[0])
                if idx not in seen:
                    ch = ot.Cell.child(par, idx)
                    seen[idx] = len(cc)
                    cc.append(ch.c); cwid.append(ch.w); pc.append(p); born.append(s); died.append(api.INT32_MAX)
    from hpmvs_amd import frontier
    snap = frontier.OctreeSnapshot(tree.root.c, tree.root.w, np.array(cc), np.array(cwid), np.array(pc), np.array(born), np.array(died))

    # the restatement replays the operations; snapshots of the tree at each odd position are taken lazily in order
    import copy
    state = {"done": 0}
    t2 = ot.OctTree(tree.root.c, tree.root.w, P_all)
    t2.root = copy.deepcopy(tree.root)
    leaves_t2 = t2.nonempty()
    assert len(leaves_t2) == L0 and all((a.c == b.c).all() for a, b in zip(leaves_t2, leaves0))

    def tree_at(q):
        while state["done"] < len(ops) and ops[state["done"]][1] < q:
            kind, s, v, pts = ops[state["done"]]
            leaf = leaves_t2[v]
            if kind == "remove":
                t2.remove(leaf)
            else:
                t2.split(leaf)
                for e in pts:
                    t2.at(P_all[e], leaf).data.append(e)
            state["done"] += 1
        return t2

    # cells: expanded patches, each at an odd position; in position order (the restatement advances monotonically)
    n_cells = min(R.n, 2 * n_ops + 1)
    cells = [int(i) for i in rng.permutation(R.n)[:n_cells]]
    position = np.array(sorted(rng.choice(np.arange(1, 2 * n_ops + 1, 2), size=n_cells)), np.int32)
    expanded = np.ones(n_cells, np.uint8)
    flat_in = np.full(n_cells, -1.0, np.float32)
    cell_leaf = {i: owner[i] for i in cells}
    fl, nn = _compare("versioned", gpu_scene, t2, R, xax, cells, cell_leaf, expanded, flat_in, snap, position, trees_at=tree_at)
    # the same cells against the table WITHOUT versioning (the tree at the sweep's start) differ somewhere
    static = frontier.OctreeSnapshot(snap.root_center, snap.root_width, snap.cell_center[:L0], snap.cell_width[:L0], snap.patch_center[:L0])
    idx = np.array(cells)
    sub = api.Batch(R.center[idx], R.normal[idx], R.scale[idx], R.n_images[idx], R.images[idx])
    cw = np.array([cell_leaf[i].w for i in cells], np.float32)
    fl0, nn0, _ = frontier.regularize_level(gpu_scene, sub, cw, position, expanded, static, flat_in)
    differ = int(((fl0.view(np.int32) != fl.view(np.int32)) | (nn0 != nn)).sum())
    print("versioned: ops", len(ops), "cells", n_cells, "differ from the start-of-sweep tree:", differ)
    assert differ > 0


def _raw_call(gscene, R, cw, snap):
    """hpmvs_regularize_batch through ctypes, returning the status and the output arrays as the call left them."""
    import ctypes as C
    from hpmvs_amd import api
    n = R.n
    t = api.LeafTable()
    t.n = snap.n
    for k in range(3):
        t.root_center[k] = float(snap.root_center[k])
    t.root_width = float(snap.root_width)
    t.cell_center, t.cell_width, t.patch_center = snap.cell_center.ctypes.data, snap.cell_width.ctypes.data, snap.patch_center.ctypes.data
    t.born, t.died = snap.born.ctypes.data, snap.died.ctypes.data
    pos = np.zeros(n, np.int32); exp = np.ones(n, np.uint8)
    fl = np.full(n, -7.0, np.float32); nn = np.full(n, -9, np.int32); nb = np.full((n, 24), -9, np.int32)
    b = R.c_struct()
    rc = api.lib().hpmvs_regularize_batch(gscene.h, C.byref(b), cw.ctypes.data, pos.ctypes.data, exp.ctypes.data, C.byref(t),
                                          fl.ctypes.data, nn.ctypes.data, nb.ctypes.data, 0, None)
    return rc, fl, nn, nb


def test_malformed_leaf_tables_are_refused_before_any_write(tiny_scene, gpu_scene):
    from hpmvs_amd import api, frontier
    rng = np.random.default_rng(3)
    R = _refined(tiny_scene, gpu_scene, 200, 61)
    tree, _ = _build(R, rng, dup=0.0)
    leaves = tree.nonempty()
    snap = _table(tree, leaves)
    cw = np.array([tree.at(tree.P[i]).w for i in range(R.n)], np.float32)
    rc, fl, nn, nb = _raw_call(gpu_scene, R, cw, snap)
    assert rc == 0 and (nn >= 0).all()
    # one leaf centre one ulp off the grid
    bad = frontier.OctreeSnapshot(snap.root_center, snap.root_width, snap.cell_center.copy(), snap.cell_width, snap.patch_center)
    bad.cell_center[len(leaves) // 2, 1] = np.nextafter(bad.cell_center[len(leaves) // 2, 1], np.float32(np.inf))
    # a leaf 22 levels below the root (its centre on the grid: the recurrence followed down to a patch)
    deep = ot.Cell(tree.root.c, tree.root.w)
    p = tree.P[0]
    for _ in range(22):
        idx = (int(p[2] > deep.c[2]) << 2) | (int(p[1] > deep.c[1]) << 1) | int(p[0] > deep.c[0])
        deep = ot.Cell.child(deep, idx)
        if _ == 20:
            ok21 = deep
    ext = lambda c: frontier.OctreeSnapshot(snap.root_center, snap.root_width, np.concatenate([snap.cell_center, c.c[None]]),
                                            np.concatenate([snap.cell_width, [c.w]]), np.concatenate([snap.patch_center, p[None]]))
    # a width that is no power-of-two fraction of the root's
    odd = frontier.OctreeSnapshot(snap.root_center, snap.root_width, snap.cell_center, snap.cell_width * np.float32(0.75), snap.patch_center)
    for name, t in (("off the grid", bad), ("depth 22", ext(deep)), ("width", odd)):
        rc, fl, nn, nb = _raw_call(gpu_scene, R, cw, t)
        assert rc == -2, (name, rc)   # HPMVS_ERR_ARG
        assert (fl == -7.0).all() and (nn == -9).all() and (nb == -9).all(), name
    rc, fl, nn, nb = _raw_call(gpu_scene, R, cw, ext(ok21))   # depth 21 is the deepest a path key holds
    assert rc == 0
