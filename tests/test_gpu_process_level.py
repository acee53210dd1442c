"""One sweep of processCell over cells of mixed flatness (reference src/hpmvs/CellProcessor.cpp:369-420: regularize for flatness_ < 0,
removal for flatness_ > 2.4, branch otherwise) as hpmvs_amd.frontier.process_level -- ONE settle pass and ONE regularize pass
against the versioned tree -- against the sequential loop: per cell, orc.branch_round on its one leaf, OracleDepths.set_depths(p,
true) for removals, and the float32 restatement of regularize (tests/octree_ref.py) on the restated DynOctTree as it stands at
the cell's turn.  After the sweep: flatness bits, removed / split / children, the nonempty leaves (cell and data[0]) and every
depth map are equal.
Scope: ONE sweep over a random queue whose flatness_ values are set (-1: regularize, 0: branch, 2.5 / 2.6: removal), not the full
seeds -> extend -> x1 -> x2 -> extend chain; removals come from set values, not from a flatness regularize computed.  Off-surface
outliers supply the 2.5 / 2.6 results of regularize, and branched leaves neighbour regularized ones, so versioning is exercised
(asserted: some cells differ from the tree at the sweep's start)."""
import numpy as np
import pytest

import octree_ref as ot

pytestmark = pytest.mark.gpu


def _oracle_patch(batch, k):
    from oracle import oracle as orc
    arr = (orc.Patch * 1)()
    p = arr[0]
    p.center[:] = batch.center[k].tolist(); p.normal[:] = batch.normal[k].tolist()
    p.scale = float(batch.scale[k])
    p.n_images = int(batch.n_images[k])
    for i in range(p.n_images):
        p.images[i] = int(batch.images[k, i])
    return arr


def _maps_equal(gpu_scene, OD, n_views, n_levels):
    from hpmvs_amd import api
    for v in range(n_views):
        for l in range(n_levels):
            if not np.array_equal(api.depth_level(gpu_scene, v, l), OD.level(v, l)):
                return False, (v, l)
    return True, None


def _sweep(tag, scene, gscene, oscene, n_seeds, seed_off):
    from hpmvs_amd import api, frontier, synth
    from oracle import oracle as orc
    rng = np.random.default_rng(seed_off)
    seeds = synth.make_seeds(scene, n_seeds, start_level=2, seed=synth.SEED + seed_off)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gscene, b)
    keep = np.nonzero(b.ok)[0]
    R = api.Batch(b.center[keep], b.normal[keep], b.scale[keep], b.n_images[keep], b.images[keep])
    # off-surface outliers: copies of patches moved six leaf widths along their normal (isolated leaves: flatness 2.5 / 2.6)
    k_out = max(8, R.n // 20)
    pick = rng.permutation(R.n)[:k_out]
    nrm = R.normal[pick, :3] / np.linalg.norm(R.normal[pick, :3], axis=1, keepdims=True)
    oc = R.center[pick].copy()
    oc[:, :3] += (nrm * (6.0 * R.scale[pick, None] * 2.0 / 0.9)).astype(np.float32)
    R = api.Batch(np.concatenate([R.center, oc]), np.concatenate([R.normal, R.normal[pick]]), np.concatenate([R.scale, R.scale[pick]]),
                  np.concatenate([R.n_images, R.n_images[pick]]), np.concatenate([R.images, R.images[pick]]))
    outlier = np.zeros(R.n, bool)
    outlier[-k_out:] = True
    xax = [np.array(api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height, 5).xaxis[:], np.float32) for v in scene.views]
    # the tree: every refined patch added at its own scale (leaves on several levels), one patch per leaf (the first)
    P = R.center[:, :3].astype(np.float32)
    lo, hi = P.min(axis=0), P.max(axis=0)
    rc = ((lo + hi) / 2).astype(np.float32)
    rw = np.float32(2.0 ** np.ceil(np.log2(float((hi - lo).max()) * 1.1)))
    width = (R.scale * np.float32(2.0 / 0.9) * np.exp2(rng.integers(0, 2, size=R.n))).astype(np.float32)
    tree = ot.OctTree(rc, rw, P)
    for e in rng.permutation(R.n):
        tree.add(int(e), width[e])
    leaves = tree.nonempty()
    for l in leaves:
        del l.data[1:]
    # the queue: a random order; flatness_ 0 (a patch that was never regularized: settle -> branch), -1 (regularize), and some
    # off-surface outliers given 2.5 / 2.6 (removal)
    order = rng.permutation(len(leaves))
    leaves = [leaves[j] for j in order]
    cells_idx = np.array([l.data[0] for l in leaves])
    n = len(leaves)
    fl0 = np.where(rng.random(n) < 0.5, -1.0, 0.0).astype(np.float32)
    rem = rng.random(n) < 0.08
    fl0[rem] = np.where(rng.random(int(rem.sum())) < 0.5, 2.5, 2.6).astype(np.float32)
    fl0[outlier[cells_idx]] = -1.0
    final = (rng.random(n) < 0.3).astype(np.uint8)
    cells = api.Batch(R.center[cells_idx], R.normal[cells_idx], R.scale[cells_idx], R.n_images[cells_idx], R.images[cells_idx])
    snap = frontier.OctreeSnapshot(rc, rw, np.array([l.c for l in leaves]), np.array([l.w for l in leaves]), P[cells_idx])
    n_levels = oscene.camera(0).n_levels
    # the maps before the sweep: every leaf's patch entered
    api.depth_reset(gscene)
    cells.ok[:] = 1
    api.set_depths_batch(gscene, cells)
    OD = orc.OracleDepths(oscene)
    OP = [_oracle_patch(cells, k) for k in range(n)]
    for k in range(n):
        OD.set_depths(OP[k][0])

    res = frontier.process_level(gscene, cells, np.arange(n), fl0, np.ones(n, np.uint8), snap, final, neighbours=True)

    # the sequential loop
    tree.P = list(P)
    fl_seq = fl0.copy()
    removed, split, children = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 4), bool)
    n_at_start_differs = 0
    import copy
    start_tree = copy.deepcopy(tree)
    start_tree.P = P
    for q in range(n):
        leaf = leaves[q]
        if fl0[q] < 0:
            want, found = ot.regularize(tree, cells.center[q], cells.normal[q], xax[int(cells.images[q, 0])], leaf.w, True, fl0[q])
            fl_seq[q] = want
            w0, _ = ot.regularize(start_tree, cells.center[q], cells.normal[q], xax[int(cells.images[q, 0])], leaf.w, True, fl0[q])
            n_at_start_differs += np.float32(w0).tobytes() != np.float32(want).tobytes()
        elif float(fl0[q]) > 2.4:
            OD.set_depths(OP[q][0], subtract=True)
            tree.remove(leaf)
            removed[q] = 1
        else:
            cand, sp = orc.branch_round(oscene, OD, OP[q], leaf.c[None], np.array([leaf.w], np.float32), final[q:q + 1], which=orc.OPT_REF)
            if sp[0]:
                split[q] = 1
                tree.split(leaf)
                for k in range(4):
                    if cand[k].stage == 0:
                        children[q, k] = True
                        c = np.array(cand[k].center[:3], dtype=np.float32)
                        tree.P.append(c)
                        tree.at(c, leaf).data.append(len(tree.P) - 1)
    tree.P = np.array(tree.P, np.float32)

    st = res.settled
    assert np.array_equal(res.flatness.view(np.int32), fl_seq.view(np.int32)), (tag, np.nonzero(res.flatness != fl_seq)[0][:10])
    assert np.array_equal(res.settle.removed, removed[st]) and np.array_equal(res.settle.split, split[st])
    assert np.array_equal(res.settle.children, children[st])
    # the nonempty leaves after the sweep: those of the versioned table alive at the end
    alive = res.snapshot.died == api.INT32_MAX
    got = sorted((res.snapshot.cell_center[j].tobytes(), res.snapshot.cell_width[j].tobytes(), res.snapshot.patch_center[j].tobytes())
                 for j in np.nonzero(alive)[0])
    want = sorted((np.asarray(l.c, np.float32).tobytes(), np.float32(l.w).tobytes(), tree.P[l.data[0]].tobytes()) for l in tree.nonempty())
    assert got == want, (tag, len(got), len(want))
    ok, where = _maps_equal(gscene, OD, scene.n_views, n_levels)
    assert ok, (tag, where)
    rep = {"cells": n, "removed": int(removed.sum()), "split": int(split.sum()), "children": int(children.sum()),
           "flat_2.5": int((fl_seq[fl0 < 0] == np.float32(2.5)).sum()), "flat_2.6": int((fl_seq[fl0 < 0] == np.float32(2.6)).sum()),
           "regularized": int((fl0 < 0).sum()), "differs_from_start_tree": int(n_at_start_differs)}
    print("process level", tag, rep)
    for k in ("removed", "split", "children", "flat_2.5", "flat_2.6", "differs_from_start_tree"):
        assert rep[k] > 0, (tag, k)


def test_process_level_equals_the_sequential_loop_on_configs0(tiny_scene, oracle_scene, gpu_scene):
    _sweep("configs0_3v_640x480", tiny_scene, gpu_scene, oracle_scene, 700, 71)


def test_process_level_equals_the_sequential_loop_on_a_12_view_scene():
    from hpmvs_amd import api, synth
    from oracle import oracle as orc
    scene = synth.make_scene(12, 640, 480, n_waves=24)
    g = api.Scene(scene, device=0)
    try:
        _sweep("12v_640x480", scene, g, orc.OracleScene(scene), 900, 73)
    finally:
        g.close()
