"""One priority level of the expansion as a FRONTIER -- batched on the GPU -- with the reference's SEQUENTIAL result.

Reference: main.cpp:146-181 pops the leaves of one priority level and CellProcessor::extend (CellProcessor.cpp:84-178) runs
on them one after the other: candidate -> octree pre-gate (:118-122) -> optimize -> scale / drift gates (:124-128) ->
the three depth-map counts (:130-139, Scene.cpp:518-644) -> DynOctTree::addConditional (doctree.h:397-419) ->
Scene::setDepths (Scene.cpp:351-381).  Candidate i's counts are read from maps that the candidates accepted BEFORE it in the
same level have already written, and its octree cell may have been taken by one of them.

`extend_level` keeps that meaning and the batching.  There is ONE walk in this module (`_candidates`, `_level`, `_walk`); the
level's queue holds the candidates in the reference's order and, for `filter_extend_level`, SUBTRACTION EVENTS between them
(the patches CellProcessor::filter removed from a cell, right before that cell's candidates).  `extend_level` is the walk
without events.
  * ONE hpmvs_expand_batch refines every candidate of the level (the refinement reads neither the maps nor the octree);
  * ONE hpmvs_level_conflicts_batch gives the level's conflict graph: which refined candidate's setDepths, or which event's
    setDepths(p, true), would write a map cell that another refined candidate's gates read or another node writes (a candidate
    that was not refined reads and writes none).  The cells themselves stay on the device; `_walk` is handed one token per
    conflicting pair in place of the pair's common cells;
  * the queue is then decided in WAVES.  A wave = one hpmvs_depth_gates_batch over the still undecided candidates against the
    maps as they are, a walk over the pending items in the reference's order, one ordered depth update for what was accepted
    (hpmvs_set_depths_batch when the wave holds additions only, else ONE hpmvs_depth_ops_batch in queue order: subtracting a
    depth does not commute with adding one).
    In the walk a candidate is DECIDED (accepted or rejected for good) unless something it depends on is still open:
      - a map cell it reads may be written by an earlier item of this walk: a candidate that was accepted or deferred, an event
        applied or deferred (`dirty`: its counts were read before that write),
      - a cell it would write is read by an earlier deferred candidate (that one must not see this write later) or written by
        an earlier deferred event (the addition must follow the subtraction) (`guard`),
      - its octree cell (before or after refinement) is the possible cell of an earlier deferred candidate (`maybe_occ`),
        or an earlier deferred candidate looks at the cell it would occupy (`occ_guard`);
    then it is DEFERRED to the next wave, and leaves its own possible effects in those sets.
    An EVENT always passes and occupies no leaf.  It is deferred when one of its cells is written by an earlier candidate
    accepted or deferred in this wave (`cand_dirty`), or read by an earlier deferred candidate (`cand_guard`); events never
    block each other (subtractions commute).  Applied or deferred, its cells join `dirty`; deferred, they also join `guard`.
    The first undecided item of a wave always gets decided (the sets are empty when it is reached), so the waves end; their
    number is the depth of the dependency chains, not the number of candidates (tests/test_gpu_expand_round.py records it: a
    handful).
  The result -- stage codes, counts, accepted set, occupancy, every depth map -- equals the sequential loop's, candidate by
  candidate (asserted against the oracle's `orc_extend_round` on BASELINE configs[0] and on a 12-view scene; with events
  against the sequential filter / extend loop, tests/test_gpu_filter_level.py).  tests/test_cpu_frontier_walk.py
  drives `_walk` without a device against the sequential loop of a toy model.
  Every level call takes device_walk=True: the queue then goes to ONE hpmvs_level_walk_batch, which runs the waves on the device
  by the same rule stated over earlier neighbours (hpmvs_amd/csrc/level_walk.hpp), and `_walk` is not
  used.  `_walk` stays the readable statement of the rule and the default.

The octree itself stays with the scheduler (out of scope): `occupied` is the caller's set of cell keys,
`cell_key` the caller's map from a point to its leaf (default: the uniform grid of leaf width `width`).
Stage codes as in hpmvs_expand_batch, plus 20 = leaf already taken (no refinement), 23 / 24 / 25 = depthTests /
viewBlockTest / pixelFreeTests threshold, 26 = addConditional found the refined patch's leaf taken.

`extend_level_tree` / `filter_extend_level_tree` are the same walk against the REAL octree (`Octree`: branch keys + nonempty leaf
keys, looked up on the device inside ONE hpmvs_extend_tree_batch per level): the pre-gate sees leaves of any depth, addConditional splits, and a
candidate that ends outside the tree's root is a border candidate, stage 27.

`extend_level_forest` / `filter_extend_level_forest` run that walk ONCE over the queues of all subtrees of a `partition`, one after
the other, with ONE hpmvs_extend_forest_batch for the candidates of every tree: the per-tree loop's result in list order, border
patches delivered between levels.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import api


def cell_key(p, width) -> int:
    """Key of the grid cell floor(p / width) per axis (float32 division, as a leaf look-up on the refined centre)."""
    w = np.float32(width)
    ix, iy, iz = (int(np.floor(np.float32(p[k]) / w)) for k in range(3))
    return ((ix + (1 << 20)) << 42) | ((iy + (1 << 20)) << 21) | (iz + (1 << 20))


def _cell(view, level, x, y):
    return (((int(view) << 3) | int(level)) << 48) | ((int(x) & 0xFFFFFF) << 24) | (int(y) & 0xFFFFFF)


def _full_depth_cells(view, ix0, iy0, n_levels, out):
    """Cells Scene::getFullDepth visits for the 3x3 level-0 pixel block from (ix0, iy0) (Scene.cpp:406-432, 538-550):
    (pixel / DEPTH_SUBSAMPLE) >> level on every level.  Pixels outside the image are never looked up; keeping them would
    only add keys that no write can have."""
    seen = set()
    for py in (iy0, iy0 + 1, iy0 + 2):
        if py < 0:
            continue
        for px in (ix0, ix0 + 1, ix0 + 2):
            if px < 0:
                continue
            c0 = (px >> 1, py >> 1)
            if c0 in seen:
                continue
            seen.add(c0)
            x, y = c0
            for l in range(n_levels):
                out.add(_cell(view, l, x, y))
                x >>= 1; y >>= 1


@dataclass
class LevelResult:
    candidates: api.Batch          # the 6 n candidates (refined where they were refined)
    stage: np.ndarray              # final stage code per candidate (0 = accepted and inserted)
    counts: np.ndarray             # [6 n, 3] depthTests / viewBlockTest / pixelFreeTests at decision time (-1: not reached)
    accepted: list                 # candidate indices in the reference's order
    waves: int                     # gate / setDepths passes it took
    deferred_per_wave: list = field(default_factory=list)
    border: list = field(default_factory=list)   # extend_level_tree: the stage-27 candidates in queue order (the scheduler routes them)
    leaf_key: dict = field(default_factory=dict)  # extend_level_tree: accepted candidate -> path key of the leaf it went into
    tree: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))   # extend_level_forest: the tree of every candidate


MAX_LEVELS = 8                     # HPMVS_MAX_LEVELS


def _rows(b: api.Batch, idx, width=None) -> api.Batch:
    idx = np.asarray(idx, dtype=np.int64)
    img = b.images[idx]
    if width is not None and width > img.shape[1]:
        img = np.pad(img, ((0, 0), (0, width - img.shape[1])), constant_values=-1)
    return api.Batch(b.center[idx], b.normal[idx], b.scale[idx], b.n_images[idx], img)


def _concat(batches) -> api.Batch:
    return api.Batch(*[np.concatenate([getattr(b, f) for b in batches]) for f in ("center", "normal", "scale", "n_images", "images")])


def _pyramid_levels(scene: api.Scene, who: str) -> int:
    """The deepest pyramid of the scene's cameras: the levels getFullDepth walks, so the levels a read can be on."""
    n_levels = max(scene.view_levels) if scene.view_levels else 1
    if n_levels > MAX_LEVELS:
        raise ValueError(f"{who}: the scene's cameras have {n_levels} pyramid levels, more than HPMVS_MAX_LEVELS")
    return n_levels


class _GridKeys:
    """The candidates' leaves on the caller's uniform grid (`key`, default cell_key) with the caller's `occupied` set."""

    def __init__(self, key, width, occupied):
        self.key, self.width, self.occupied = key, width, occupied

    def pre(self, center):
        pre_key = [self.key(c, self.width) for c in center]
        return pre_key, np.array([k in self.occupied for k in pre_key], np.uint8)   # level-start occupancy: those are never refined

    def post(self, center, refined):
        return [self.key(center[t], self.width) if refined[t] else None for t in range(len(center))], None

    def candidates(self, scene, parents, width, o):
        """Two hpmvs_expand_batch calls: everything skipped (constructed only) for the centres before optimize -> their cells,
        then the refinement of those whose cell is free when the level starts."""
        n = parents.n
        N = 6 * n
        cc = np.zeros((n, 3), np.float32)
        widths = np.full(n, width, np.float32)
        pre = api.expand_batch(scene, api.EXPAND_EXTEND, parents, cc, widths, np.ones(N, np.uint8), options=o)
        pre_key, skip = self.pre(pre.center)
        out = api.expand_batch(scene, api.EXPAND_EXTEND, parents, cc, widths, skip, options=o)
        refined = (out.stage == 0) & (skip == 0)
        post_key, border = self.post(out.center, refined)
        return out, pre_key, post_key, skip, refined, border


def _candidates(scene, parents, width, keys, o):
    """The candidate steps of a level, the keys object's business as a whole: the six candidates of every parent before optimize
    and their leaves (`pre_key`), the refinement of those whose leaf is free when the level starts (`skip`: the others), the
    refined ones' leaves (`post_key`) and, on the real tree, the refined ones that left the root (`border`, else None).
    `keys`: _GridKeys (two hpmvs_expand_batch calls) or _TreeKeys (ONE hpmvs_extend_tree_batch)."""
    return keys.candidates(scene, parents, width, o)


def _walk(queue, pre_key, post_key, refined, n_images, reads, writes, ev_cells, occupied, min_images, stage, counts, gates, apply,
          sequential=True, border=None):
    """The wave walk of the module docstring over `queue`: items ("c", t) (candidate t) and ("e", j) (subtraction event j) in the
    reference's order.  reads(t) / writes(t): the map cells refined candidate t's gates read / its setDepths would write (sets);
    ev_cells[j]: the cells event j writes.  The device is reached through two callables only: gates(list of candidates) -> their
    (depthTests, viewBlockTest, pixelFreeTests) counts from the maps as they are, apply(ops) enters a wave's accepted candidates
    and applied events, given as queue items in queue order.  `stage` (preset to each candidate's refinement result) and `counts`
    are filled in place, `occupied` grows.  Returns (accepted in queue order, waves, deferred per wave).  sequential = False
    drops every deferral of a candidate (one wave; meaningful without events only).
    border: the refined candidates that lie outside the tree's root (a set, or flags indexed by candidate; default none).  Such
    a candidate waits on its reads like any other and, past the three counts, gets stage 27: it writes no depth and occupies no
    leaf (its post_key is never looked at), so while deferred it only guards what it reads."""
    MIN = min_images
    is_border = (lambda t: False) if border is None else (lambda t: t in border) if isinstance(border, (set, frozenset)) \
        else (lambda t: bool(border[t]))
    accepted, waves, deferred_log = [], 0, []
    pending = list(queue)
    while pending:
        waves += 1
        todo = [t for kind, t in pending if kind == "c" and refined[t]]
        cnt = dict(zip(todo, gates(todo))) if todo else {}
        dirty, guard, maybe_occ, occ_guard = set(), set(), set(), set()
        cand_dirty, cand_guard = set(), set()     # the candidates' share of dirty / guard: what an event checks
        deferred, ops = [], []

        def defer(t):
            deferred.append(("c", t))
            occ_guard.add(pre_key[t])
            if refined[t]:
                guard.update(reads(t)); cand_guard.update(reads(t))
                if not is_border(t):
                    dirty.update(writes(t)); cand_dirty.update(writes(t))
                    maybe_occ.add(post_key[t]); occ_guard.add(post_key[t])

        for kind, t in pending:
            if kind == "e":
                c = ev_cells[t]
                dirty.update(c)
                if not c.isdisjoint(cand_dirty) or not c.isdisjoint(cand_guard):
                    deferred.append(("e", t))
                    guard.update(c)
                else:
                    ops.append(("e", t))
                continue
            pk = pre_key[t]
            if pk in occupied:
                stage[t] = 20                       # its leaf was taken (by an earlier candidate: occupancy only grows in order)
                continue
            if sequential and pk in maybe_occ:
                defer(t)
                continue
            if not refined[t]:
                continue                            # failed in optimize or at the scale / drift gates (its preset stage): reads no map
            if sequential and not reads(t).isdisjoint(dirty):
                defer(t)
                continue
            v_, b_, f_ = cnt[t]
            counts[t] = (v_, b_, f_)
            if not v_ >= MIN:
                stage[t] = 23
            elif not b_ < MIN:
                stage[t] = 24
            elif not (f_ >= MIN - 1 and f_ * 1.0 / n_images[t] > 0.75):
                stage[t] = 25
            elif is_border(t):
                stage[t] = 27                       # handed to borderCellFn_: not inserted, no depths
            else:
                k_ = post_key[t]
                if k_ in occupied:
                    stage[t] = 26
                elif sequential and (k_ in maybe_occ or k_ in occ_guard or not writes(t).isdisjoint(guard)):
                    counts[t] = (-1, -1, -1)
                    defer(t)
                else:
                    occupied.add(k_)
                    stage[t] = 0
                    accepted.append(t); ops.append(("c", t))
                    dirty.update(writes(t)); cand_dirty.update(writes(t))
        if ops:
            apply(ops)
        deferred_log.append(len(deferred))
        pending = deferred
    return accepted, waves, deferred_log


def _walk_key(k):
    """A leaf key of the walk as hpmvs_level_walk_batch takes it: (set or None, 64-bit key).  The grid's and a tree's keys are
    integers, a forest's (tree, key) pairs; REFUSED is key 0 of whatever set."""
    return (int(k[0]), int(k[1])) if isinstance(k, tuple) else (None, int(k))


def _device_walk(scene, out, events, n_ev, M, queue, pre_key, post_key, skip, refined, border, occupied, margin, abs_int, o):
    """The walk of `queue` as ONE hpmvs_level_walk_batch: the queue's items become the rows of one batch with
    their flag bytes, sets and keys -- no graph, no token set and no count reaches the host -- and the call's arrays fill the
    LevelResult `_walk` would have filled.  `occupied` grows by the accepted candidates' leaves."""
    N = out.n
    n = len(queue)
    flags, sets = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    pre, post = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    rows = np.zeros(n, np.int64)
    for i, (kind, t) in enumerate(queue):
        if kind == "e":
            flags[i], rows[i] = api.WALK_EVENT, N + t
            continue
        rows[i] = t
        f, s = 0, None
        pk = pre_key[t]
        if not (isinstance(pk, tuple) and pk[0] == "outside"):     # (an outside candidate is never pre-gated)
            s, pre[i] = _walk_key(pk)
            f |= api.WALK_HAS_PRE | (api.WALK_PRE_TAKEN if pk in occupied else 0)
        if refined[t]:
            f |= api.WALK_REFINED
            if border is not None and border[t]:
                f |= api.WALK_BORDER
            else:
                s2, post[i] = _walk_key(post_key[t])
                s = s if s2 is None else s2
                f |= api.WALK_POST_TAKEN if post_key[t] in occupied else 0
        flags[i], sets[i] = f, 0 if s is None else s
    both = _concat([_rows(out, np.arange(N), M)] + ([_rows(events, np.arange(n_ev), M)] if n_ev else []))
    stage = np.where(skip != 0, 20, out.stage).astype(np.int32)
    counts = np.full((N, 3), -1, np.int32)
    cand = np.array([kind == "c" for kind, _ in queue], bool)
    st, cnt, acc, wave, waves = api.level_walk(scene, _rows(both, rows), flags, sets, pre, post, margin, abs_int, o,
                                               stage=np.where(cand, stage[np.minimum(rows, N - 1)], 0) if n else None)
    stage[rows[cand]] = st[cand]
    counts[rows[cand]] = cnt[cand]
    accepted = sorted(int(t) for t in rows[cand & (acc != 0)])
    for t in accepted:
        occupied.add(post_key[t])
    deferred_log = [int((wave > w + 1).sum()) for w in range(waves)]
    return LevelResult(out, stage, counts, accepted, waves, deferred_log, [t for kind, t in queue if kind == "c" and stage[t] == 27],
                       {t: post_key[t] for t in accepted} if border is not None else {})


def _level(scene, parents, width, occupied, margin, abs_int, o, keys, n_levels, sequential=True, events=None, event_cell=(), walk="host"):
    """CellProcessor::extend over `parents` with the subtraction events `events` (a Batch, or None): event j comes before the
    candidates of parent event_cell[j] (non-decreasing).  The candidate steps, the queue, ONE hpmvs_level_conflicts_batch over the
    queue's events and refined candidates, and the walk with the device behind its two callables.  `n_levels` is not used: the
    call takes the pyramid levels from the scene's cameras, as _pyramid_levels does.
    walk = "device": the candidate steps and the queue as before, then ONE hpmvs_level_walk_batch in place of the graph call, the
    token sets and `_walk` (_device_walk); the LevelResult is the same."""
    out, pre_key, post_key, skip, refined, border = _candidates(scene, parents, width, keys, o)
    N = 6 * parents.n
    rc = np.nonzero(refined)[0]
    n_ev = events.n if events is not None else 0
    M = max(out.max_images, events.max_images) if n_ev else out.max_images
    # the queue: per parent its events, then its six candidates
    queue = []
    j = 0
    for i in range(parents.n):
        while j < n_ev and event_cell[j] == i:
            queue.append(("e", j))
            j += 1
        queue.extend(("c", t) for t in range(6 * i, 6 * i + 6) if not skip[t])
    if walk == "device":
        if not sequential:
            raise ValueError("the device walk is the sequential walk: sequential = False has no device form")
        return _device_walk(scene, out, events, n_ev, M, queue, pre_key, post_key, skip, refined, border, occupied, margin, abs_int, o)
    if walk != "host":
        raise ValueError(f"walk must be 'host' or 'device', not {walk!r}")
    # The level's conflict graph from ONE hpmvs_level_conflicts_batch over the nodes in queue order (the events and the refined
    # candidates): no footprint and no cell key reaches the host.  _walk only ever intersects one node's reads /
    # writes with other nodes' writes / reads, so every conflicting pair gets ONE token, in both sets it is a member of: ("rw",
    # writer, reader) in the writer's writes (an event's ev_cells) and in the reader's reads, ("ww", candidate, event) in the
    # candidate's writes and in the event's ev_cells.  Every intersection test then has the truth value it has over cells.
    nodes = [(kind, t) for kind, t in queue if kind == "e" or refined[t]]
    both = _concat([_rows(out, rc, M)] + ([_rows(events, np.arange(n_ev), M)] if n_ev else []))
    at_row = {int(t): i for i, t in enumerate(rc)}
    fp = _rows(both, [len(rc) + t if kind == "e" else at_row[t] for kind, t in nodes])
    is_ev = np.array([kind == "e" for kind, _ in nodes], np.uint8)
    read_tok, write_tok = [set() for _ in nodes], [set() for _ in nodes]
    if fp.n:
        flow_off, flow_adj, anti_off, anti_adj = api.level_conflicts(scene, fp, is_ev if n_ev else None)
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
    node_of = {t: i for i, (kind, t) in enumerate(nodes) if kind == "c"}
    reads = lambda t: read_tok[node_of[t]]
    writes = lambda t: write_tok[node_of[t]]
    ev_cells = [None] * n_ev
    for i, (kind, t) in enumerate(nodes):
        if kind == "e":
            ev_cells[t] = write_tok[i]

    def gates(todo):
        v, b, f = api.depth_gates_batch(scene, _rows(out, todo), margin, abs_int)
        return [(int(v[i]), int(b[i]), int(f[i])) for i in range(len(todo))]

    def apply(ops):
        # additions only: hpmvs_set_depths_batch; with a subtraction ONE hpmvs_depth_ops_batch in queue order
        sub = np.array([kind == "e" for kind, _ in ops], np.uint8)
        batch = _rows(out, [t for kind, t in ops if kind == "c"], M)
        if sub.any():
            both = _concat([batch, _rows(events, [t for kind, t in ops if kind == "e"], M)])
            batch = _rows(both, np.argsort(np.argsort(sub, kind="stable")))   # back from (additions, subtractions) to queue order
        batch.ok[:] = 1
        if sub.any():
            api.depth_ops_batch(scene, batch, sub)
        else:
            api.set_depths_batch(scene, batch)

    stage = np.where(skip != 0, 20, out.stage).astype(np.int32)
    counts = np.full((N, 3), -1, np.int32)
    accepted, waves, deferred_log = _walk(queue, pre_key, post_key, refined, out.n_images, reads, writes, ev_cells, occupied,
                                          int(o.MIN_IMAGES_PER_PATCH), stage, counts, gates, apply, sequential, border)
    return LevelResult(out, stage, counts, sorted(accepted), waves, deferred_log, [t for kind, t in queue if kind == "c" and stage[t] == 27],
                       {t: post_key[t] for t in accepted} if border is not None else {})


def _walk_mode(device_walk) -> str:
    return "device" if device_walk else "host"


def extend_level(scene: api.Scene, parents: api.Batch, width: float, occupied: set, margin: float = 1.0, abs_int: int = 0,
                 options=None, n_levels: int = 6, key=cell_key, sequential: bool = True, device_walk: bool = False) -> LevelResult:
    """CellProcessor::extend over `parents` (the leaves of one priority level, in the scheduler's order): the walk of the module
    docstring without events.  `occupied` is updated in place; the scene's depth maps receive the accepted candidates.
    sequential = False gives round 3's plain frontier round (every count read from the maps as they are when the level starts):
    one wave, not the reference's result when candidates of a level interact through the maps.
    `n_levels` is kept for existing callers and ignored: the pyramid levels a read can be on are the scene's cameras' (at most
    HPMVS_MAX_LEVELS, ValueError beyond), so no value given here can hide a read from the walk.
    device_walk = True (here and in the other level calls): the waves run inside ONE hpmvs_level_walk_batch instead of `_walk` on
    the host; the result is the same, field for field."""
    return _level(scene, parents, width, occupied, margin, abs_int, options or api.default_options(), _GridKeys(key, width, occupied),
                  _pyramid_levels(scene, "extend_level"), sequential, walk=_walk_mode(device_walk))


@dataclass
class BranchResult:
    candidates: api.Batch          # the 4 n children (refined where they were refined; stage 20: not built / not refined)
    support: np.ndarray            # Scene::getLevelSupport of every leaf's patch
    split: np.ndarray              # [n] 1: the leaf was split (its patch's depths taken back, the children's entered)
    children: np.ndarray           # [n, 4] bool: the children that go into the new leaves


def branch_level(scene: api.Scene, parents: api.Batch, cell_center, cell_width, final_level, options=None) -> BranchResult:
    """One priority level of CellProcessor::branch (reference CellProcessor.cpp:210-307) over `parents` -- the patches of the
    level's leaves, in the scheduler's order -- as ONE hpmvs_level_support_batch (the first gate, :221-224), ONE
    hpmvs_expand_batch (the four diagonal children, Cell::contains before and after optimize, :233-258: the refinement reads
    neither the maps nor the tree) and ONE hpmvs_depth_ops_batch that replays the leaves' map updates in the reference's
    order: per split leaf its patch's depths taken back (:276-279), then its children's entered (:296) -- subtraction does not
    commute with the minimum, so the order is part of the result.  `final_level[i]`: nodeLevel(leaf i) >= PATCH_FINAL_MINLEVEL
    (the scheduler's knowledge): such a leaf keeps its patch when no child survived (:265-266).  The tree operations (split,
    the children's leaves, the queue) stay with the caller; the result names what to do.  Equals the sequential loop's
    (`orc_branch_round`): children, split decisions, every depth map (tests/test_gpu_branch_level.py).
    settle_level with no leaf above the removal threshold."""
    r = settle_level(scene, parents, cell_center, cell_width, np.zeros(parents.n, np.float32), final_level, options)
    return BranchResult(r.candidates, r.support, r.split, r.children)


REMOVE_FLATNESS = 2.4   # processCell (CellProcessor.cpp:409): flatness_ > 2.4 removes the patch


def child_cell(center, width, idx):
    """Cell(parent, idx) (doctree.cpp:30-36): width_ = parent width / 2.0, c_[k] = parent c_[k] +- width_ / 2.0, computed in
    double and stored as float."""
    w = np.float32(float(width) / 2.0)
    c = np.array([float(center[k]) + (1.0 if (idx >> k) & 1 else -1.0) * float(w) / 2.0 for k in range(3)], dtype=np.float32)
    return c, w


def octant(center, p) -> int:
    """Branch::at's child index (doctree.h:250-255): bit k set where p[k] > c_[k]."""
    return (int(np.float32(p[2]) > np.float32(center[2])) << 2) | (int(np.float32(p[1]) > np.float32(center[1])) << 1) | \
        int(np.float32(p[0]) > np.float32(center[0]))


@dataclass
class SettleResult:
    candidates: api.Batch          # the 4 n branch children (stage 20: not built / not refined, removed leaves included)
    support: np.ndarray            # Scene::getLevelSupport of every leaf's patch
    removed: np.ndarray            # [n] 1: flatness_ > 2.4, the patch was removed (its depths taken back, the leaf emptied)
    split: np.ndarray              # [n] 1: the leaf was split (its patch's depths taken back, the children's entered)
    children: np.ndarray           # [n, 4] bool: the children that go into the new leaves
    child_octant: np.ndarray       # [n, 4] the octant of the split leaf each child goes into (-1: not a child)
    octant_center: np.ndarray      # [n, 8, 3] Cell::c_ of the split leaf's eight children


def settle_level(scene: api.Scene, parents: api.Batch, cell_center, cell_width, flatness, final_level, options=None) -> SettleResult:
    """processCell's decision for expanded leaves with flatness_ >= 0 (reference CellProcessor.cpp:409-419), in the scheduler's
    order: flatness_ > 2.4 removes the patch (Scene::setDepths(p, true), the leaf emptied), anything else goes to
    CellProcessor::branch.  ONE hpmvs_level_support_batch and ONE hpmvs_expand_batch (the removed leaves' children are skipped),
    then ONE hpmvs_depth_ops_batch in queue order that interleaves the removals' subtractions with the branches' subtractions
    and additions: subtracting a depth does not commute with other depth updates.  The tree operations stay with the caller:
    the result says per leaf removed / split and which child goes into which child leaf."""
    o = options or api.default_options()
    n = parents.n
    cc = np.ascontiguousarray(cell_center, dtype=np.float32).reshape(n, 3)
    cw = np.ascontiguousarray(cell_width, dtype=np.float32).reshape(n)
    final = np.ascontiguousarray(final_level).astype(bool).reshape(n)
    fl = np.ascontiguousarray(flatness, dtype=np.float32).reshape(n)
    removed = fl.astype(np.float64) > REMOVE_FLATNESS    # float > double, as the reference compares
    support = api.level_support_batch(scene, parents, int(o.MINLEVEL))
    skip = np.repeat((support < 1) | removed, 4).astype(np.uint8)   # an exhausted or removed leaf builds nothing
    out = api.expand_batch(scene, api.EXPAND_BRANCH, parents, cc, cw, skip, options=o)
    children = ((out.stage == 0) & (skip == 0)).reshape(n, 4)
    split = ~removed & (support >= 1) & ~(final & (children.sum(axis=1) == 0))
    # the map updates in the reference's order: leaf by leaf, a removed patch out, or the old patch out and the children in
    M = max(parents.max_images, out.max_images)
    widen = lambda a: np.pad(a, ((0, 0), (0, M - a.shape[1])), constant_values=-1)
    rows_c, rows_n, rows_s, rows_m, rows_i, sub = [], [], [], [], [], []
    pimg, cimg = widen(parents.images), widen(out.images)
    for i in np.nonzero(split | removed)[0]:
        rows_c.append(parents.center[i]); rows_n.append(parents.normal[i]); rows_s.append(parents.scale[i])
        rows_m.append(parents.n_images[i]); rows_i.append(pimg[i]); sub.append(1)
        if removed[i]:
            continue
        for k in np.nonzero(children[i])[0]:
            t = 4 * i + k
            rows_c.append(out.center[t]); rows_n.append(out.normal[t]); rows_s.append(out.scale[t])
            rows_m.append(out.n_images[t]); rows_i.append(cimg[t]); sub.append(0)
    if sub:
        ops = api.Batch(np.array(rows_c), np.array(rows_n), np.array(rows_s), np.array(rows_m), np.array(rows_i))
        ops.ok[:] = 1
        api.depth_ops_batch(scene, ops, np.array(sub, np.uint8))
    child_octant = np.full((n, 4), -1, np.int32)
    octant_center = np.zeros((n, 8, 3), np.float32)
    for i in np.nonzero(split)[0]:
        for idx in range(8):
            octant_center[i, idx] = child_cell(cc[i], cw[i], idx)[0]
        for k in np.nonzero(children[i])[0]:
            child_octant[i, k] = octant(cc[i], out.center[4 * i + k])
    return SettleResult(out, support, removed.astype(np.uint8), split.astype(np.uint8), children, child_octant, octant_center)


@dataclass
class OctreeSnapshot:
    """The scheduler's octree as hpmvs_regularize_batch reads it: the root Branch and the nonempty leaves, each valid at queue
    positions born < q < died (include/hpmvs_amd.h: hpmvs_leaf_table)."""
    root_center: np.ndarray        # [3] Cell::c_ of the root Branch (a subtree's root when the model is split)
    root_width: float
    cell_center: np.ndarray        # [L, 3] Leaf::c_
    cell_width: np.ndarray         # [L]
    patch_center: np.ndarray       # [L, 3] data[0]->center_
    born: np.ndarray = None        # [L] (default -1)
    died: np.ndarray = None        # [L] (default INT32_MAX)

    def __post_init__(self):
        self.cell_center = np.ascontiguousarray(self.cell_center, dtype=np.float32).reshape(-1, 3)
        L = len(self.cell_center)
        self.cell_width = np.ascontiguousarray(self.cell_width, dtype=np.float32).reshape(L)
        self.patch_center = np.ascontiguousarray(np.asarray(self.patch_center, dtype=np.float32)[:, :3]).reshape(L, 3)
        self.born = np.full(L, -1, np.int32) if self.born is None else np.ascontiguousarray(self.born, dtype=np.int32).reshape(L)
        self.died = np.full(L, api.INT32_MAX, np.int32) if self.died is None else np.ascontiguousarray(self.died, dtype=np.int32).reshape(L)

    @property
    def n(self):
        return len(self.cell_width)


def regularize_level(scene: api.Scene, cells: api.Batch, cell_width, position, expanded, snapshot: OctreeSnapshot, flatness=None,
                     neighbours: bool = False):
    """CellProcessor::regularize (reference CellProcessor.cpp:309-367) for the cells of a level as ONE hpmvs_regularize_batch:
    cell i sees the tree as it stands at its queue position position[i].  Returns (flatness, n_neighbours, neighbour_leaf)."""
    t = snapshot
    return api.regularize_batch(scene, cells, cell_width, position, expanded, t.root_center, t.root_width, t.cell_center,
                                t.cell_width, t.patch_center, t.born, t.died, flatness=flatness, neighbours=neighbours)


@dataclass
class ProcessResult:
    flatness: np.ndarray           # [n] flatness_ after the sweep (regularized cells updated, the others as given)
    n_neighbours: np.ndarray       # [n] neighbour leaves of the regularized cells (-1: not expanded, -2: settled)
    neighbour_leaf: np.ndarray     # [n, 24] their snapshot indices (None unless asked for)
    settled: np.ndarray            # indices of the cells settle_level decided (flatness_ >= 0)
    settle: SettleResult           # its result, row j for cell settled[j]
    snapshot: OctreeSnapshot       # the versioned tree of the sweep: the split children's leaves appended, died / born set
    child_leaf: np.ndarray         # [len(settled), 4] snapshot index of the leaf each child went into (-1: none)


def process_level(scene: api.Scene, cells: api.Batch, cell_leaf, flatness, expanded, snapshot: OctreeSnapshot, final_level,
                  options=None, neighbours: bool = False) -> ProcessResult:
    """One sweep of processCell over cells of mixed flatness (priority L*10 + 1 / + 2, CellProcessor.cpp:390-419), in the
    scheduler's order (queue position = index): cell_leaf[i] is the snapshot index of cell i's leaf.  (1) settle_level on the
    cells with flatness_ >= 0, (2) their removals and splits become died / born entries of the versioned tree, (3)
    regularize_level on the cells with flatness_ < 0 against it.  regularize only reads the tree and settle does not read
    flatness, so one pass of each gives the sequential loop's result."""
    n = cells.n
    fl = np.ascontiguousarray(flatness, dtype=np.float32).reshape(n).copy()
    leaf = np.ascontiguousarray(cell_leaf, dtype=np.int64).reshape(n)
    final = np.ascontiguousarray(final_level).astype(bool).reshape(n)
    exp = np.ascontiguousarray(expanded).astype(np.uint8).reshape(n)
    # processCell extends an unexpanded cell instead (:386-392), and one leaf changes at most once per sweep (died / born)
    if not exp.all():
        raise ValueError("process_level: every cell must be expanded (an unexpanded one goes to extend_level)")
    if len(np.unique(leaf)) != n or (n and (leaf.min() < 0 or leaf.max() >= snapshot.n)):
        raise ValueError("process_level: every cell must own a distinct leaf of the snapshot")
    reg = fl < 0
    settled = np.nonzero(~reg)[0]                   # (NaN is not < 0: processCell settles it)
    t = snapshot
    S = settle_level(scene, _rows(cells, settled), t.cell_center[leaf[settled]], t.cell_width[leaf[settled]], fl[settled],
                     final[settled], options)
    cc, cw, pc = [t.cell_center], [t.cell_width], [t.patch_center]
    born, died = [t.born], [t.died.copy()]
    child_leaf = np.full((len(settled), 4), -1, np.int64)
    L = t.n
    for j, i in enumerate(settled):
        if S.removed[j] or S.split[j]:
            died[0][leaf[i]] = i
        if not S.split[j]:
            continue
        w = np.float32(float(t.cell_width[leaf[i]]) / 2.0)
        new = {}
        for k in range(4):                          # data[0] of a child leaf: its first child (branch pushes in k order)
            o_ = int(S.child_octant[j, k])
            if o_ < 0:
                continue
            if o_ not in new:
                new[o_] = L
                cc.append(S.octant_center[j, o_][None]); cw.append(np.array([w], np.float32))
                pc.append(S.candidates.center[4 * j + k, :3][None])
                born.append(np.array([i], np.int32)); died.append(np.array([api.INT32_MAX], np.int32))
                L += 1
            child_leaf[j, k] = new[o_]
    snap = OctreeSnapshot(t.root_center, t.root_width, np.concatenate(cc), np.concatenate(cw), np.concatenate(pc),
                          np.concatenate(born), np.concatenate(died))
    nn = np.full(n, -2, np.int32)
    nb = np.full((n, api.REGULARIZE_PROBES), -1, np.int32) if neighbours else None
    ri = np.nonzero(reg)[0]
    if len(ri):
        f_, n_, b_ = regularize_level(scene, _rows(cells, ri), snap.cell_width[leaf[ri]], ri, exp[ri], snap, fl[ri], neighbours)
        fl[ri] = f_; nn[ri] = n_
        if neighbours:
            nb[ri] = b_
    return ProcessResult(fl, nn, nb, settled, S, snap, child_leaf)


@dataclass
class FilterResult:
    keep: np.ndarray               # [n_cells] row of the kept patch (-1: empty cell, -2: no winner)
    dist: np.ndarray               # [n] the reference's mean signed plane distance per row (0 in single-patch cells)
    removed: np.ndarray            # [n] 1: a loser (its depths taken back, its images_ cleared by the caller)


def _cell_offsets(patches: api.Batch, cell_start) -> np.ndarray:
    cs = np.ascontiguousarray(cell_start, dtype=np.int64).reshape(-1)
    if len(cs) < 1 or cs[0] != 0 or cs[-1] != patches.n or (np.diff(cs) < 0).any():
        raise ValueError("cell_start must start at 0, not decrease and end at the number of patches")
    return cs.astype(np.int32)


def _filter(scene: api.Scene, patches: api.Batch, cell_start) -> FilterResult:
    cs = _cell_offsets(patches, cell_start)
    dist, keep = api.filter_batch(scene, patches, cs)
    if (keep == -2).any():
        raise ValueError(f"filter: cell {int(np.nonzero(keep == -2)[0][0])} has no patch whose distance is below FLT_MAX "
                         "(the reference would keep a null pointer)")
    removed = np.ones(patches.n, np.uint8)
    removed[keep[keep >= 0]] = 0
    return FilterResult(keep, dist, removed)


def filter_level(scene: api.Scene, patches: api.Batch, cell_start, options=None) -> FilterResult:
    """CellProcessor::filter (reference CellProcessor.cpp:43-82) for the cells of a level, in the scheduler's order: cell c holds
    the rows cell_start[c] .. cell_start[c + 1] - 1 of `patches` in data order.  ONE hpmvs_filter_batch, then ONE
    hpmvs_depth_ops_batch that takes the losers' depths back in queue order (Scene::setDepths(p, true)).  The result is the
    sequential loop's when nothing else runs between the filters; processCell's first visit, which extends each kept patch right
    after its filter, is filter_extend_level.  Raises ValueError before the maps are touched when a cell has no winner.
    (`options`: the signature of the other level calls; filter reads none.)"""
    r = _filter(scene, patches, cell_start)
    losers = np.nonzero(r.removed)[0]
    if len(losers):
        ops = _rows(patches, losers)
        ops.ok[:] = 1
        api.depth_ops_batch(scene, ops, np.ones(len(losers), np.uint8))
    return r


def filter_extend_level(scene: api.Scene, patches: api.Batch, cell_start, width: float, occupied: set, expanded=None,
                        margin: float = 1.0, abs_int: int = 0, options=None, key=cell_key, device_walk: bool = False):
    """processCell's first visit of a level's unexpanded leaves (reference CellProcessor.cpp:369-392), in queue order: filter
    cell i (:377-378), then CellProcessor::extend on its kept patch.  Returns (FilterResult, LevelResult); the LevelResult is laid
    out as extend_level's, the kept patches being the parents.

    ONE hpmvs_filter_batch decides every cell (filter reads only the cell's own patches).  Then the walk of the module docstring
    over the kept patches, each loser a subtraction event at its queue position (after the candidates of the cells before it,
    before its own cell's candidates); always sequential.  The result equals the sequential loop's; on a level
    of single-patch cells there are no events and it is extend_level's, wave for wave.

    `expanded`: expanded_ per row (default 0).  ValueError before any map update for a cell with no winner, an empty cell or a
    kept patch that is already expanded (processCell does not extend it, :380)."""
    return _filter_extend(scene, patches, cell_start, width, _GridKeys(key, width, occupied), occupied, expanded, margin, abs_int,
                          options, "filter_extend_level", device_walk)


def _filter_extend(scene, patches, cell_start, width, keys, occupied, expanded, margin, abs_int, options, who, device_walk=False):
    n_levels = _pyramid_levels(scene, who)
    cs = _cell_offsets(patches, cell_start)
    exp = np.zeros(patches.n, np.uint8) if expanded is None else np.ascontiguousarray(expanded).astype(np.uint8).reshape(patches.n)
    if (np.diff(cs) == 0).any():
        raise ValueError(f"{who}: cell {int(np.nonzero(np.diff(cs) == 0)[0][0])} is empty")
    F = _filter(scene, patches, cs)
    if exp[F.keep].any():
        raise ValueError(f"{who}: the kept patch of cell {int(np.nonzero(exp[F.keep])[0][0])} is already expanded")
    losers = np.nonzero(F.removed)[0]
    cell_of = np.repeat(np.arange(len(cs) - 1), np.diff(cs))
    L = _level(scene, _rows(patches, F.keep), width, occupied, margin, abs_int, options or api.default_options(), keys, n_levels,
               events=_rows(patches, losers), event_cell=cell_of[losers], walk=_walk_mode(device_walk))
    return F, L


@dataclass
class SeedTree:
    """The octree Scene::initPatches leaves behind (reference Scene.cpp:183-199), as the level calls read it: the nonempty leaves
    in Leaf_iterator order and the batch rows they hold, in data order."""
    root_center: np.ndarray        # [3] Cell::c_ of the root Branch
    root_width: float
    scale_floor: float             # width / (1 << PATCH_INIT_MAXLEVEL + 1): no scale_3dx_ lies below it afterwards
    rows: np.ndarray               # [n_rows] rows of the batch with ok != 0, leaf by leaf
    cell_start: np.ndarray         # [n_leaves + 1] leaf l holds rows[cell_start[l] : cell_start[l + 1]]
    cell_center: np.ndarray        # [n_leaves, 3] Leaf::c_
    cell_width: np.ndarray         # [n_leaves]
    cell_level: np.ndarray         # [n_leaves] nodeLevel
    patch_center: np.ndarray       # [n_leaves, 3] data[0]->center_

    @property
    def n_leaves(self):
        return len(self.cell_width)

    def snapshot(self) -> OctreeSnapshot:
        """The tree as regularize_level / process_level read it: every leaf present from the start (born -1, died INT32_MAX)."""
        return OctreeSnapshot(self.root_center, self.root_width, self.cell_center, self.cell_width, self.patch_center)

    def cells(self, batch: api.Batch) -> api.Batch:
        """The rows of `batch` gathered in cell order: with cell_start, what filter_level / filter_extend_level take."""
        out = _rows(batch, self.rows)
        out.ok[:] = 1
        return out


def seed_tree(scene: api.Scene, batch: api.Batch, patch_init_maxlevel: int = 9, set_depths: bool = True) -> SeedTree:
    """The second half of Scene::initPatches for the survivors (ok != 0) of `batch`, e.g. of api.init_patches_batch, in row order:
    ONE hpmvs_seed_tree_batch.  batch.scale receives the scale floor; with set_depths the scene's depth maps (api.depth_reset
    first) receive the survivors' depths."""
    info, rows, cs, cc, cw, cl, pc = api.seed_tree_batch(scene, batch, patch_init_maxlevel, set_depths)
    R, L = int(info.n_rows), int(info.n_leaves)
    return SeedTree(np.array(info.root_center, np.float32), float(info.root_width), float(info.scale_floor), rows[:R].copy(),
                    cs[:L + 1].copy(), cc[:L].copy(), cw[:L].copy(), cl[:L].copy(), pc[:L].copy())


# ---- the level calls against the real octree -------------------------------------------------------

MAX_TREE_DEPTH = api.OCTREE_MAX_DEPTH


def key_depth(key: int) -> int:
    """Levels of a path key below the root (the root is 1: depth 0)."""
    return (int(key).bit_length() - 1) // 3


class Octree:
    """The scheduler's DynOctTree (reference include/hpmvs/doctree.h) as hpmvs_octree_locate_batch reads it: the set of branch
    keys and a dict nonempty leaf key -> the caller's row.  Path keys: a sentinel bit, then 3 bits per level (z y x, Branch::at's
    child test x > c_); the root Branch is key 1 and implicit.  An empty leaf is a key in neither container whose parent is a
    branch.  Cells follow from the root by Cell(parent, idx) (double arithmetic, float storage).  The host operations have the
    reference's meaning; a row is whatever the caller keeps per leaf (an index, a list of patches)."""
    ROOT = 1

    def __init__(self, root_center, root_width, root_level: int = 0):
        self.root_center = np.array(root_center, dtype=np.float32).reshape(3)
        self.root_width = np.float32(root_width)
        self.root_level = int(root_level)      # rootLevel_: nodeLevel of the root (a subtree keeps the level of its cut)
        self.branches = set()
        self.leaves = {}
        self._below = {}                       # branch key -> nonempty leaves below it
        self._cells = {self.ROOT: (self.root_center, self.root_width)}

    # -- cells
    def cell(self, key: int):
        """(c_, width_) of the cell with path `key`."""
        c = self._cells.get(key)
        if c is None:
            pc, pw = self.cell(key >> 3)
            c = self._cells[key] = child_cell(pc, pw, key & 7)
        return c

    def node_level(self, key: int) -> int:
        """DynOctTree::nodeLevel: log2(root width / width) + rootLevel_."""
        return key_depth(key) + self.root_level

    def contains(self, p) -> bool:
        """getRoot()->contains(p) (doctree.cpp:38-42): hw = width_ / 2.0 as float; > below, <= above."""
        hw = np.float32(float(self.root_width) / 2.0)
        c = self.root_center
        q = [np.float32(p[k]) for k in range(3)]
        return bool(all(q[k] > np.float32(c[k] - hw) for k in range(3)) and all(q[k] <= np.float32(c[k] + hw) for k in range(3)))

    def at(self, p, start: int = ROOT) -> int:
        """root->at(p): the key of the leaf (of any depth, empty or not) that p descends to, whatever p is."""
        key = start
        while True:
            key = (key << 3) | octant(self.cell(key)[0], p)
            if key not in self.branches:
                return key

    def row(self, key: int):
        return self.leaves.get(key)

    # -- changes
    def _count(self, key: int, d: int):
        k = key >> 3
        while k:
            self._below[k] = self._below.get(k, 0) + d
            k >>= 3

    def insert(self, key: int, row):
        """Put `row` into the EMPTY leaf `key`, creating the branches on the way (what addConditional's splits leave behind)."""
        if not 1 <= key_depth(key) <= MAX_TREE_DEPTH or key in self.branches or key in self.leaves:
            raise ValueError(f"Octree.insert: {key:#x} is a branch, a nonempty leaf or no key within {MAX_TREE_DEPTH} levels")
        k = key >> 3
        while k != self.ROOT:
            if k in self.leaves:
                raise ValueError(f"Octree.insert: {key:#x} lies below the nonempty leaf {k:#x}")
            self.branches.add(k)
            k >>= 3
        self.leaves[key] = row
        self._count(key, +1)

    def split(self, key: int):
        """Leaf::split: the leaf becomes a Branch with eight empty leaves; its row (None for an empty leaf) is returned."""
        if key in self.branches or key_depth(key) >= MAX_TREE_DEPTH or (key >> 3) != self.ROOT and (key >> 3) not in self.branches:
            raise ValueError(f"Octree.split: {key:#x} is no leaf that can be split")
        row = self.leaves.pop(key, None)
        if row is not None:
            self._count(key, -1)
        self.branches.add(key)
        return row

    def add_conditional(self, p, width, row):
        """DynOctTree::addConditional(p, width) (doctree.h:397-419): None when p's leaf is nonempty or narrower than `width`,
        else the key of the leaf `row` went into, after splitting while leaf width / 2.0 > width."""
        width = np.float32(width)
        key = self.at(p)
        if key in self.leaves or self.cell(key)[1] < width:
            return None
        while key_depth(key) < MAX_TREE_DEPTH and float(self.cell(key)[1]) / 2.0 > float(width):
            self.branches.add(key)
            key = (key << 3) | octant(self.cell(key)[0], p)
        self.leaves[key] = row
        self._count(key, +1)
        return key

    def remove(self, key: int) -> int:
        """DynOctTree::remove(leaf) (doctree.h:422-450): the leaf is cleared; when its parent Branch is then empty all through, the
        parent becomes ONE empty leaf (remove_internal collapses one level only; the root stays a Branch).  Returns the key of
        the leaf that is there afterwards."""
        if self.leaves.pop(key, None) is not None:
            self._count(key, -1)
        par = key >> 3
        if par == self.ROOT or self._below.get(par, 0):
            return key
        self._drop(par)
        return par

    def _drop(self, key: int):
        self.branches.discard(key)
        self._below.pop(key, None)
        for i in range(8):
            if ((key << 3) | i) in self.branches:
                self._drop((key << 3) | i)

    # -- views
    @staticmethod
    def _aligned(key: int) -> int:
        d = key_depth(key)
        return (key ^ (1 << (3 * d))) << (3 * (MAX_TREE_DEPTH - d))

    def leaf_table(self):
        """The nonempty leaves in Leaf_iterator order (children 0 .. 7, depth first): (keys [L] uint64, rows (list), cell_center
        [L, 3], cell_width [L])."""
        keys = sorted(self.leaves, key=self._aligned)
        cc = np.array([self.cell(k)[0] for k in keys], np.float32).reshape(len(keys), 3)
        cw = np.array([self.cell(k)[1] for k in keys], np.float32)
        return np.array(keys, np.uint64), [self.leaves[k] for k in keys], cc, cw

    def snapshot(self, patch_center) -> "OctreeSnapshot":
        """The tree as regularize_level reads it; patch_center[l]: data[0]->center_ of leaf l of leaf_table()."""
        _, _, cc, cw = self.leaf_table()
        return OctreeSnapshot(self.root_center, float(self.root_width), cc, cw, patch_center)

    def branch_keys(self) -> np.ndarray:
        return np.array(sorted(self.branches), np.uint64)

    def subtree(self, key: int) -> "Octree":
        """The tree below the branch `key`, re-rooted there (the reference's subtrees, DynOctTree::swapRoot): keys re-based, the
        root's level kept for nodeLevel."""
        if key != self.ROOT and key not in self.branches:
            raise ValueError(f"Octree.subtree: {key:#x} is no branch")
        d = key_depth(key)
        c, w = self.cell(key)
        sub = Octree(c, w, self.root_level + d)

        def rebase(k):
            dk = key_depth(k) - d
            return (k & ((1 << (3 * dk)) - 1)) | (1 << (3 * dk)) if dk > 0 and (k >> (3 * dk)) == key else 0

        sub.branches = {rebase(k) for k in self.branches} - {0}
        for k, row in self.leaves.items():
            if rebase(k):
                sub.leaves[rebase(k)] = row
                sub._count(rebase(k), +1)
        return sub

    @classmethod
    def from_seed_tree(cls, tree: "SeedTree") -> "Octree":
        """The tree right after Scene::initPatches: leaf l of `tree` under the key its cell_center descends to in cell_level[l]
        levels, row l; the branches are all proper prefixes (add() only ever splits)."""
        t = cls(tree.root_center, tree.root_width)
        for l in range(tree.n_leaves):
            key = cls.ROOT
            for _ in range(int(tree.cell_level[l])):
                key = (key << 3) | octant(t.cell(key)[0], tree.cell_center[l])
            if t.cell(key)[1] != tree.cell_width[l]:
                raise ValueError(f"Octree.from_seed_tree: leaf {l} is not a cell of the root's subdivision")
            t.insert(key, l)
        return t

    def locate(self, scene: api.Scene, points, add_width=None) -> api.OctreeLocation:
        """ONE hpmvs_octree_locate_batch against the tree as it stands (leaf_index: into leaf_table())."""
        return api.octree_locate_batch(scene, self.root_center, self.root_width, self.branch_keys(), self.leaf_table()[0], points, add_width)

    def insert_batch(self, scene: api.Scene, points, add_width, rows):
        """addConditional(points[i], add_width[i]) for i = 0 .. n - 1 in that order as ONE hpmvs_octree_insert_batch against the
        tree as it stands (every patch sees the earlier ones' leaves), then insert(key, rows[i]) for the accepted patches in
        queue order.  Returns api.OctreeInsertion (accepted, leaf_key, blocker: include/hpmvs_amd.h)."""
        r = api.octree_insert_batch(scene, self.root_center, self.root_width, self.branch_keys(), self.leaf_table()[0], points, add_width)
        for i in np.nonzero(r.accepted)[0]:
            self.insert(int(r.leaf_key[i]), rows[i])
        return r


REFUSED = 0   # no path key: what addConditional's refusal maps to; in `occupied` from the start of a level


class _TreeKeys:
    """The candidates' leaves in the real tree: ONE hpmvs_extend_tree_batch per level builds, looks up, refines and looks up
    again.  Within a level every parent has the same width w, an exact level width of the tree, so addConditional(0.9 w) ends at
    the depth d* of width w: whatever the tree as the level finds it decides is static (a nonempty leaf, or structure finer than
    w: never refined / REFUSED), and whatever the level's own insertions decide is equality of the d*-prefix of the point -- the
    walk's pre_key / post_key."""

    def __init__(self, scene, tree: Octree, width):
        self.scene, self.tree = scene, tree
        self.width = np.float32(width)
        w, d = tree.root_width, 0
        while w > self.width and d < MAX_TREE_DEPTH:
            w = np.float32(float(w) / 2.0); d += 1
        if w != self.width or d < 1:
            raise ValueError("extend_level_tree: `width` is not the width of a level of the tree")
        self.index = (tree.branch_keys(), tree.leaf_table()[0])

    def candidates(self, scene, parents, width, o):
        t = self.tree
        out, k = api.extend_tree_batch(scene, parents, self.width, t.root_center, t.root_width, self.index[0], self.index[1], options=o)
        N = out.n
        refined = (out.stage == 0) & (k.skip == 0)
        border = refined & (k.border != 0)                                              # CellProcessor.cpp:147
        # an outside candidate is never pre-gated: a key that nothing else can hold
        pre_key = [int(k.pre_key[t]) if k.pre_inside[t] else ("outside", t) for t in range(N)]
        post_key = [None if not refined[t] else ("border", t) if border[t] else int(k.post_key[t]) for t in range(N)]
        return out, pre_key, post_key, k.skip, refined, border


def _insert_accepted(tree: Octree, L: LevelResult, rows):
    for k, t in enumerate(L.accepted):
        tree.insert(L.leaf_key[t], rows[k] if rows is not None else ("extend", t))


def extend_level_tree(scene: api.Scene, parents: api.Batch, width: float, tree: Octree, margin: float = 1.0, abs_int: int = 0,
                      options=None, sequential: bool = True, events=None, event_cell=(), rows=None,
                      device_walk: bool = False) -> LevelResult:
    """extend_level against the scheduler's real octree (or a subtree of it): CellProcessor::extend over `parents`, the leaves
    of ONE node level (all of width `width`), in the scheduler's order.  The walk is extend_level's; the candidates and their keys come
    from ONE hpmvs_extend_tree_batch (_TreeKeys).  Stage codes as extend_level's, where 20 is the pre-gate (a nonempty leaf of any
    depth, or structure finer than `width`, inside the root), 26 addConditional's refusal, and 27 = BORDER: a candidate that
    passed every gate but lies outside tree's root.  Border candidates are returned in LevelResult.border (queue order) for the
    scheduler to route (processBorderCellQueue); they are not inserted and write no depths.  The accepted candidates are
    inserted into `tree` at LevelResult.leaf_key, with the branches on the way, under rows[k] for the k-th accepted (default a
    ("extend", candidate) tuple).  events / event_cell: subtraction events as in filter_extend_level."""
    keys = _TreeKeys(scene, tree, width)
    L = _level(scene, parents, width, {REFUSED}, margin, abs_int, options or api.default_options(), keys,
               _pyramid_levels(scene, "extend_level_tree"), sequential, events, event_cell, _walk_mode(device_walk))
    _insert_accepted(tree, L, rows)
    return L


def filter_extend_level_tree(scene: api.Scene, patches: api.Batch, cell_start, width: float, tree: Octree, expanded=None,
                             margin: float = 1.0, abs_int: int = 0, options=None, rows=None, device_walk: bool = False):
    """filter_extend_level against the real octree: the same walk with extend_level_tree's keys, the filters' losers as events.
    Returns (FilterResult, LevelResult)."""
    keys = _TreeKeys(scene, tree, width)
    F, L = _filter_extend(scene, patches, cell_start, width, keys, {REFUSED}, expanded, margin, abs_int, options,
                          "filter_extend_level_tree", device_walk)
    _insert_accepted(tree, L, rows)
    return F, L


# ---- a level over all subtrees at once --------------------------------------------------------------

def _flatten_forest(trees):
    """A list of Octree as hpmvs_octree_forest takes it: (roots [n, 4], branch_first, leaf_first, branch_key, leaf_key), every
    tree's leaves in leaf_table() order."""
    n = len(trees)
    bk = [t.branch_keys() for t in trees]
    lk = [t.leaf_table()[0] for t in trees]
    roots = np.array([[*t.root_center, t.root_width] for t in trees], np.float32).reshape(n, 4)
    branch_first = np.concatenate([[0], np.cumsum([len(a) for a in bk])]).astype(np.int32)
    leaf_first = np.concatenate([[0], np.cumsum([len(a) for a in lk])]).astype(np.int32)
    branch_key = np.concatenate(bk + [np.zeros(0, np.uint64)]).astype(np.uint64)
    leaf_key = np.concatenate(lk + [np.zeros(0, np.uint64)]).astype(np.uint64)
    return roots, branch_first, leaf_first, branch_key, leaf_key


class _ForestKeys:
    """_TreeKeys for a list of Octree objects: ONE hpmvs_extend_forest_batch per level serves every tree.  The walk's leaf keys
    are (tree, key) pairs, so equal sub-keys of two subtrees stay distinct; a refusal stays REFUSED whatever the tree, and
    "outside" / "border" keep their per-candidate tuples.  A tree with parents must have the level; one without may be rooted
    anywhere (a subtree rooted below the level is the normal case after getSubTrees)."""

    def __init__(self, scene, trees, parent_tree, width):
        self.scene, self.trees = scene, list(trees)
        self.width = np.float32(width)
        self.parent_tree = np.ascontiguousarray(parent_tree, dtype=np.int32).reshape(-1)
        n = len(self.trees)
        if len(self.parent_tree) and (self.parent_tree.min() < 0 or self.parent_tree.max() >= n):
            raise ValueError("extend_level_forest: a parent's tree is outside the list of trees")
        if (np.diff(self.parent_tree) < 0).any():
            raise ValueError("extend_level_forest: parent_tree / cell_tree must not decrease (the queue is the trees' queues in list order)")
        for k in np.unique(self.parent_tree):
            w, d = self.trees[k].root_width, 0
            while w > self.width and d < MAX_TREE_DEPTH:
                w = np.float32(float(w) / 2.0); d += 1
            if w != self.width or d < 1:
                raise ValueError(f"extend_level_forest: `width` is not the width of a level of tree {int(k)}")
        self.roots, self.branch_first, self.leaf_first, self.branch_key, self.leaf_key = _flatten_forest(self.trees)

    def candidates(self, scene, parents, width, o):
        out, k = api.extend_forest_batch(scene, parents, self.parent_tree, self.width, self.roots, self.branch_first, self.leaf_first,
                                         self.branch_key, self.leaf_key, options=o)
        N = out.n
        tree = np.repeat(self.parent_tree, 6)
        pair = lambda t, key: (int(tree[t]), int(key)) if key else REFUSED
        refined = (out.stage == 0) & (k.skip == 0)
        border = refined & (k.border != 0)
        pre_key = [pair(t, k.pre_key[t]) if k.pre_inside[t] else ("outside", t) for t in range(N)]
        post_key = [None if not refined[t] else ("border", t) if border[t] else pair(t, k.post_key[t]) for t in range(N)]
        return out, pre_key, post_key, k.skip, refined, border


def _insert_accepted_forest(trees, keys: _ForestKeys, L: LevelResult, rows):
    """The walk's (tree, key) pairs back to the key in the candidate's own tree; the accepted candidates into their trees."""
    L.tree = np.repeat(keys.parent_tree, 6).astype(np.int32)
    L.leaf_key = {t: pk[1] for t, pk in L.leaf_key.items()}
    for k, t in enumerate(L.accepted):
        trees[L.tree[t]].insert(L.leaf_key[t], rows[k] if rows is not None else ("extend", t))


def extend_level_forest(scene: api.Scene, parents: api.Batch, parent_tree, width: float, trees, margin: float = 1.0,
                        abs_int: int = 0, options=None, sequential: bool = True, rows=None, device_walk: bool = False) -> LevelResult:
    """extend_level_tree for ALL subtrees of a partition in one pass: `parents` are the trees' level queues one after the other
    (parent_tree non-decreasing, ValueError otherwise), `trees` a list of Octree such as Partition.trees.  The candidates of
    every tree come from ONE hpmvs_extend_forest_batch (_ForestKeys) and go through ONE walk, whose result over the concatenated
    queue is the sequential loop's: extend_level_tree on tree 0, then tree 1, and so on, from the same starting maps, with
    candidate indices mapped through the concatenation (every field but waves / deferred_per_wave, which are the one walk's).
    LevelResult.tree names every candidate's tree; leaf_key[t] is the key in that tree, where the accepted candidate is inserted.
    Border candidates (stage 27: outside their OWN tree's root) come back in LevelResult.border for route_border / insert_border:
    they are delivered between levels, never between the subtrees of one level."""
    keys = _ForestKeys(scene, trees, parent_tree, width)
    if len(keys.parent_tree) != parents.n:
        raise ValueError("extend_level_forest: parent_tree needs one entry per parent")
    L = _level(scene, parents, width, {REFUSED}, margin, abs_int, options or api.default_options(), keys,
               _pyramid_levels(scene, "extend_level_forest"), sequential, walk=_walk_mode(device_walk))
    _insert_accepted_forest(keys.trees, keys, L, rows)
    return L


def filter_extend_level_forest(scene: api.Scene, patches: api.Batch, cell_start, cell_tree, width: float, trees, expanded=None,
                               margin: float = 1.0, abs_int: int = 0, options=None, rows=None, device_walk: bool = False):
    """filter_extend_level_tree for all subtrees in one pass: cell c (rows cell_start[c] .. cell_start[c + 1] - 1 of `patches`)
    is a leaf of trees[cell_tree[c]], cell_tree non-decreasing.  The same walk with extend_level_forest's keys, the filters'
    losers as events.  Returns (FilterResult, LevelResult)."""
    keys = _ForestKeys(scene, trees, cell_tree, width)
    if len(keys.parent_tree) != len(np.asarray(cell_start).reshape(-1)) - 1:
        raise ValueError("filter_extend_level_forest: cell_tree needs one entry per cell")
    F, L = _filter_extend(scene, patches, cell_start, width, keys, {REFUSED}, expanded, margin, abs_int, options,
                          "filter_extend_level_forest", device_walk)
    _insert_accepted_forest(keys.trees, keys, L, rows)
    return F, L


# ---- the regularize / settle sweep over all subtrees at once ----------------------------------------

@dataclass
class ForestProcessResult:
    flatness: np.ndarray           # [n] flatness_ after the sweep (regularized cells updated, the others as given)
    n_neighbours: np.ndarray       # [n] neighbour leaves of the regularized cells (-2: settled)
    neighbour_key: np.ndarray      # [n, 24] their keys in the cell's own tree, first-probe order, 0-padded (None unless asked for)
    candidates: api.Batch          # the 4 n branch children (stage 20: not built / not refined)
    support: np.ndarray            # [n] Scene::getLevelSupport of every cell's patch
    removed: np.ndarray            # [n] 1: flatness_ > 2.4, the patch was removed and the leaf emptied
    split: np.ndarray              # [n] 1: the leaf was split
    children: np.ndarray           # [n, 4] bool: the children that went into the new leaves
    child_key: np.ndarray          # [n, 4] the key in the cell's tree of the leaf child k went into (0: none)


def apply_sweep(trees, cell_tree, cell_key, removed, split, children, child_key, rows=None):
    """A sweep's removals and splits applied to the Octree objects in row order: remove(key) for a removed cell; split(key) for a
    split one and insert(child_key, row) for the FIRST child (in k order) of every new leaf -- data[0], the one regularize
    reads.  The row is rows[4 i + k], or ("branch", 4 i + k)."""
    for i in range(len(cell_key)):
        t, key = trees[int(cell_tree[i])], int(cell_key[i])
        if removed[i]:
            t.remove(key)
        elif split[i]:
            t.split(key)
            for k in range(4):
                ck = int(child_key[i][k])
                if children[i][k] and ck not in t.leaves:
                    t.insert(ck, rows[4 * i + k] if rows is not None else ("branch", 4 * i + k))


def process_level_forest(scene: api.Scene, cells: api.Batch, cell_tree, cell_key, flatness, trees, patch_center, final_level=None,
                         patch_final_minlevel=None, options=None, neighbours: bool = False, rows=None) -> ForestProcessResult:
    """process_level for ALL subtrees of a partition as ONE hpmvs_process_forest_batch: `cells` are the trees' queues one after
    the other (cell_tree non-decreasing, ValueError otherwise), cell i being data[0] of the nonempty leaf cell_key[i] of
    trees[cell_tree[i]]; `trees` a list of Octree such as Partition.trees.  The tree travels as its key sets: no cell centres, no
    snapshot.  patch_center: a function or dict from (tree, key) to data[0]->center_ of that leaf.  final_level[i]:
    nodeLevel(cell i) >= PATCH_FINAL_MINLEVEL, by default tree.node_level(key) >= patch_final_minlevel.  Equals the per-tree loop
    process_level on tree 0, then tree 1, and so on, from the same starting maps.  Afterwards the removals and splits are applied
    to the Octree objects in row order (apply_sweep)."""
    trees = list(trees)
    n = cells.n
    ct = np.ascontiguousarray(cell_tree, dtype=np.int32).reshape(-1)
    ck = np.ascontiguousarray(cell_key, dtype=np.uint64).reshape(-1)
    if len(ct) != n or len(ck) != n:
        raise ValueError("process_level_forest: cell_tree / cell_key need one entry per cell")
    if n and (ct.min() < 0 or ct.max() >= len(trees)):
        raise ValueError("process_level_forest: a cell's tree is outside the list of trees")
    if (np.diff(ct) < 0).any():
        raise ValueError("process_level_forest: cell_tree must not decrease (the queue is the trees' queues in list order)")
    if final_level is None:
        if patch_final_minlevel is None:
            raise ValueError("process_level_forest: give final_level or patch_final_minlevel")
        final_level = [trees[ct[i]].node_level(int(ck[i])) >= int(patch_final_minlevel) for i in range(n)]
    roots, bf, lf, bk, lk = _flatten_forest(trees)
    center = patch_center.__getitem__ if isinstance(patch_center, dict) else patch_center
    pc = np.zeros((len(lk), 3), np.float32)
    for t in range(len(trees)):
        for l in range(int(lf[t]), int(lf[t + 1])):
            pc[l] = np.asarray(center((t, int(lk[l]))), dtype=np.float32)[:3]
    r = api.process_forest_batch(scene, cells, ct, ck, flatness, final_level, roots, bf, lf, bk, lk, pc, options=options,
                                 neighbours=neighbours)
    apply_sweep(trees, ct, ck, r.removed, r.split, r.children, r.child_key, rows)
    return ForestProcessResult(r.flatness, r.n_neighbours, r.neighbour_key, r.candidates, r.support, r.removed, r.split,
                               r.children.astype(bool), r.child_key)


def process_level_tree(scene: api.Scene, cells: api.Batch, cell_key, flatness, tree: Octree, patch_center, final_level=None,
                       patch_final_minlevel=None, options=None, neighbours: bool = False, rows=None) -> ForestProcessResult:
    """process_level_forest for one tree; patch_center: a function or dict from the key to data[0]->center_."""
    center = patch_center.__getitem__ if isinstance(patch_center, dict) else patch_center
    return process_level_forest(scene, cells, np.zeros(cells.n, np.int32), cell_key, flatness, [tree], lambda tk: center(tk[1]),
                                final_level, patch_final_minlevel, options, neighbours, rows)


# ---- a round's border patches (reference CellProcessor.cpp:487-540) ---------------------------------

def route_border(scene: api.Scene, trees, points) -> np.ndarray:
    """CellProcessor::distributeBorderCell for every point as ONE hpmvs_octree_route_batch: the index of the first tree of
    `trees` (a list of Octree, such as the subtree()s) whose root contains it, -1 for a patch that no root contains (it is
    dropped, as in the reference)."""
    roots = np.array([[*t.root_center, t.root_width] for t in trees], np.float32).reshape(len(trees), 4)
    return api.octree_route_batch(scene, roots, points)


@dataclass
class BorderResult:
    accepted: np.ndarray           # rows of `border` that went into the tree, in queue order
    leaf_key: np.ndarray           # [len(accepted)] uint64 path key of the leaf each went into
    node_level: np.ndarray         # [len(accepted)] int32 DynOctTree::nodeLevel of that leaf
    flatness: np.ndarray           # [len(accepted)] float32 0: no regularization on border cells (CellProcessor.cpp:514)
    priority: np.ndarray           # [len(accepted)] float32 handed through for the scheduler's processing_queue
    insertion: api.OctreeInsertion  # every row's decision, leaf and blocker


def insert_border(scene: api.Scene, tree: Octree, border: api.Batch, priority, rows=None) -> BorderResult:
    """CellProcessor::processBorderCellQueue for one tree: the queued border patches `border` (queue order; routed here by
    route_border) go in with addConditional(center, scale_3dx_ * 2.0) -- ONE Octree.insert_batch --, the accepted ones write
    their depths -- ONE hpmvs_set_depths_batch: additions are a minimum, their order does not matter -- and come back with
    flatness 0 and their priorities for the scheduler's queue.  rows[i]: what the tree keeps for row i (default ("border", i))."""
    n = border.n
    priority = np.broadcast_to(np.asarray(priority, np.float32), (n,))
    add_width = np.array([float(x) * 2.0 for x in border.scale], np.float32)   # double product, narrowed by the float parameter
    r = tree.insert_batch(scene, border.center, add_width, rows if rows is not None else [("border", i) for i in range(n)])
    acc = np.nonzero(r.accepted)[0]
    if len(acc):
        batch = _rows(border, acc)
        batch.ok[:] = 1
        api.set_depths_batch(scene, batch)
    keys = r.leaf_key[acc]
    return BorderResult(acc, keys, np.array([tree.node_level(int(k)) for k in keys], np.int32), np.zeros(len(acc), np.float32),
                        priority[acc].copy(), r)


@dataclass
class BorderForestResult:
    tree: np.ndarray               # [border.n] int32 the tree every row was handed to, -1: no root contains it (dropped)
    accepted: np.ndarray           # rows of `border` that went into their tree, in queue order
    leaf_key: np.ndarray           # [len(accepted)] uint64 path key, in the row's own tree, of the leaf each went into
    node_level: np.ndarray         # [len(accepted)] int32 DynOctTree::nodeLevel of that leaf
    flatness: np.ndarray           # [len(accepted)] float32 0: no regularization on border cells (CellProcessor.cpp:514)
    priority: np.ndarray           # [len(accepted)] float32 handed through for the scheduler's processing_queue
    insertion: api.BorderForestInsertion  # every row's tree, decision, leaf and blocker


def deliver_border_forest(scene: api.Scene, trees, border: api.Batch, priority, rows=None) -> BorderForestResult:
    """route_border and the loop of insert_border over the destination trees as ONE hpmvs_border_forest_batch (DESIGN.md
    section 3.17): every row of the round's border queue `border` (push order) is handed to the first tree of `trees` (a list
    of Octree such as Partition.trees) whose root contains it, goes in with addConditional(center, scale_3dx_ * 2.0) in queue
    order among the rows of its tree, and the accepted ones write their depths.  The accepted keys are entered into their Octree
    objects in queue order under rows[i] (default ("border", i)).  The result covers the whole queue: its fields are
    BorderResult's, with `tree` beside them."""
    trees = list(trees)
    n = border.n
    priority = np.broadcast_to(np.asarray(priority, np.float32), (n,))
    r = api.border_forest_batch(scene, border, *_flatten_forest(trees), set_depths=True)
    acc = np.nonzero(r.accepted)[0]
    for i in acc:
        trees[int(r.tree[i])].insert(int(r.leaf_key[i]), rows[i] if rows is not None else ("border", int(i)))
    keys = r.leaf_key[acc]
    level = np.array([trees[int(r.tree[i])].node_level(int(r.leaf_key[i])) for i in acc], np.int32)
    return BorderForestResult(r.tree, acc, keys, level, np.zeros(len(acc), np.float32), priority[acc].copy(), r)


# ---- the split into subtrees (reference src/main.cpp:50-96, CellProcessor.cpp:422-455) --------------

@dataclass
class Partition:
    trees: list                    # Octree per subtree in the reference's list order: each equals tree.subtree(root_key[t])
    root_key: np.ndarray           # [len(trees)] uint64 the roots' path keys in `tree`
    orphans: np.ndarray            # uint64 keys of the nonempty leaves of `tree` in no subtree: no CellProcessor ever sees them
    queues: list                   # queues[t]: [(priority = node_level * 10, leaf key in trees[t])] in Leaf_iterator order
    histogram: np.ndarray          # [22] int32 cellHistogram: nonempty leaves of `tree` by depth below its root
    stop: int                      # api.PARTITION_STOP
    arrays: api.OctreePartition    # the call's arrays (leaf_order / leaf_tree: into tree.leaf_table())


def partition_from_arrays(tree: Octree, branch_key, leaf_key, rows, P: api.OctreePartition) -> Partition:
    """The host half of partition(): the subtrees as Octree objects in ONE pass over hpmvs_octree_partition's arrays P for the
    key arrays it was given (rows[i]: what `tree` keeps for leaf_key[i])."""
    n = P.n_trees
    trees = []
    for t in range(n):
        sub = Octree(P.root_cell[t, :3], P.root_cell[t, 3], tree.root_level + key_depth(int(P.root_key[t])))
        trees.append(sub)
    for j in np.nonzero(P.branch_tree >= 0)[0]:
        trees[P.branch_tree[j]].branches.add(int(P.branch_sub_key[j]))
    queues = [[] for _ in range(n)]
    for i in P.leaf_order:                                     # Leaf_iterator order: initFromTree's pushes, tree by tree
        t = P.leaf_tree[i]
        if t < 0:
            continue
        key = int(P.leaf_sub_key[i])
        trees[t].leaves[key] = rows[i]
        trees[t]._count(key, +1)
        queues[t].append((trees[t].node_level(key) * 10, key))
    orphans = np.asarray(leaf_key, np.uint64)[P.leaf_tree < 0]
    return Partition(trees, P.root_key[:n].copy(), orphans, queues, P.histogram.copy(), P.stop, P)


def partition(scene: api.Scene, tree: Octree, min_trees: int = 100, min_split_leaves: int = 100) -> Partition:
    """getSubTrees(patchTree_, subTrees, FLAGS_subtrees) of the reference's main, and the initFromTree that seeds each
    CellProcessor's queue, as ONE hpmvs_octree_partition: the subtrees in the reference's list order (the order route_border
    takes), re-rooted with root_level = the depth of the cut plus tree.root_level, the rows of `tree` carried over; they can be
    handed to route_border and extend_level_tree as they are.  min_split_leaves: the reference's 100.  `tree` is not changed.
    Leaves in no subtree (Partition.orphans) are reference behaviour: they stay in the tree, and nothing extends them."""
    bk = tree.branch_keys()
    lk, rows, _, _ = tree.leaf_table()
    P = api.octree_partition(scene, tree.root_center, tree.root_width, bk, lk, min_trees, min_split_leaves)
    return partition_from_arrays(tree, bk, lk, rows, P)


def forest_leaf_order(trees, root_key, orphans=()) -> np.ndarray:
    """The rows of all subtrees and orphans in the WHOLE tree's Leaf_iterator order, data order within a leaf: the `order` that
    makes api.ply_ext write the file scene.patchTree_.toExtPly would (reference include/hpmvs/doctree.h:526-622 walks the whole
    tree, whatever the split into subtrees).  trees[t]: an Octree whose keys are relative to root_key[t], the root's path key
    in the whole tree (Partition.trees, Partition.root_key); orphans: (whole-tree leaf key, row) pairs of the nonempty leaves in
    no subtree.  A row is a patch index or a sequence of them (a leaf's data, in order).  Every key is re-based on its root's key
    and the leaves are sorted by the aligned key Octree.leaf_table sorts by.  Host code."""
    leaves = [(int(k), row) for k, row in orphans]
    for sub, root in zip(trees, root_key):
        for k, row in sub.leaves.items():
            d = key_depth(k)
            leaves.append(((int(root) << (3 * d)) | (k ^ (1 << (3 * d))), row))
    leaves.sort(key=lambda kr: Octree._aligned(kr[0]))
    out = []
    for _, row in leaves:
        out.extend(int(r) for r in np.atleast_1d(row))
    return np.array(out, dtype=np.int32)
