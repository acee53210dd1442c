"""Test infrastructure: a numpy float32 restatement of CellProcessor::filter (reference src/hpmvs/CellProcessor.cpp:43-82), cell by
cell, and of the sequential first visit of processCell (:377-392) composed from the oracle's entries: filter -> the losers'
Scene::setDepths(p, true) -> CellProcessor::extend on the kept patch.

filter, for k = data.size() >= 2 patches: per ii, n = normal.head(3) normalized (a zero vector stays as it is), x0 = centre;
dist = 0, then for jj != ii in order dist += n . (c_jj - x0) (dot left to right: (a0 b0 + a1 b1) + a2 b2), dist /= (float)(k - 1);
the first ii with dist < best (best starting at FLT_MAX) is kept.  The rows of a cell are computed together, the jj loop in order:
the masked term of jj == ii adds +0.0, which leaves a sum that starts at +0.0 unchanged (it can never be -0.0)."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def _normalized(a):
    a = np.asarray(a, dtype=f32)
    n2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    pos = n2 > f32(0)
    n = np.sqrt(np.where(pos, n2, f32(1))).astype(f32)
    return np.where(pos[:, None], a / n[:, None], a).astype(f32)


def filter_cell(center, normal):
    """One cell (rows in data order): (dist [k] float32, kept row or None).  A single patch: dist 0, kept 0; empty: None."""
    c = np.ascontiguousarray(np.asarray(center, dtype=f32)[:, :3])
    k = len(c)
    if k == 0:
        return np.zeros(0, f32), None
    if k == 1:
        return np.zeros(1, f32), 0
    nn = _normalized(np.asarray(normal, dtype=f32)[:, :3])
    d = np.zeros(k, f32)
    rows = np.arange(k)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            b = c[j][None, :] - c                       # c_jj - x0 for every row
            t = (nn[:, 0] * b[:, 0] + nn[:, 1] * b[:, 1]) + nn[:, 2] * b[:, 2]
            d = (d + np.where(rows != j, t, f32(0))).astype(f32)
        d = (d / f32(k - 1)).astype(f32)
    best, keep = FLT_MAX, None
    for i in range(k):
        if d[i] < best:
            best, keep = d[i], i
    return d, keep


def filter_cells(center, normal, cell_start):
    """Every cell: (dist [n] float32, keep [n_cells] int32 -- the kept row, -1 for an empty cell, -2 for no winner)."""
    cs = np.asarray(cell_start, dtype=np.int64)
    n = int(cs[-1])
    dist = np.zeros(n, f32)
    keep = np.zeros(len(cs) - 1, np.int32)
    for c in range(len(cs) - 1):
        s, e = int(cs[c]), int(cs[c + 1])
        d, k = filter_cell(center[s:e], normal[s:e])
        dist[s:e] = d
        keep[c] = -1 if e == s else (-2 if k is None else s + k)
    return dist, keep


def oracle_patch(batch, k):
    """Row k of an api.Batch as a one-element oracle Patch array."""
    from oracle import oracle as orc
    arr = (orc.Patch * 1)()
    p = arr[0]
    p.center[:] = batch.center[k].tolist(); p.normal[:] = batch.normal[k].tolist()
    p.scale = float(batch.scale[k])
    p.n_images = int(batch.n_images[k])
    for i in range(p.n_images):
        p.images[i] = int(batch.images[k, i])
    return arr


def sequential_filter_extend(oscene, depths, patches, cell_start, width, occupied, margin=1.0, abs_int=0):
    """processCell's first visit of every cell in queue order, on the oracle: the restated filter, the losers' depths taken back
    one by one (orc_set_depths_ex(..., 1)), then orc_extend_round on the kept patch alone (the true sequential loop, counts from
    the live maps).  `depths` and `occupied` are updated in place.  Returns (dist, keep, candidates [6 n_cells], counts)."""
    from oracle import oracle as orc
    dist, keep = filter_cells(patches.center, patches.normal, cell_start)
    cs = np.asarray(cell_start, dtype=np.int64)
    cands, counts = [], []
    for c in range(len(cs) - 1):
        for r in range(int(cs[c]), int(cs[c + 1])):
            if r != keep[c]:
                depths.set_depths(oracle_patch(patches, r)[0], subtract=True)
        out, cnt = orc.extend_round(oscene, depths, oracle_patch(patches, int(keep[c])), width, occupied, margin, abs_int,
                                    frozen_gates=False)
        cands.extend(out[t] for t in range(6))
        counts.append(cnt)
    return dist, keep, cands, np.concatenate(counts) if counts else np.zeros((0, 3), np.int32)
