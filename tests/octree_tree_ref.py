"""Test infrastructure for the level calls on the real octree (hpmvs_octree_locate_batch, frontier.Octree, extend_level_tree):
  * Tree: tests/octree_ref.py's pointer tree with Cell::contains (doctree.cpp:38-42) and DynOctTree::addConditional
    (doctree.h:397-419), and its image as path keys;
  * HostOctree: hpmvs_amd/csrc/octree.hpp compiled by g++ (tests/octree_host.cpp) into a directory the caller chooses;
  * sequential_extend: CellProcessor::extend (CellProcessor.cpp:84-178) over the parents of one level, candidate by candidate on
    the LIVE pointer tree and the oracle's live depth maps."""
import ctypes as C
import os
import subprocess

import numpy as np

import octree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "octree_host.cpp")
f32 = np.float32
MAX_DEPTH = 21
OUTPUTS = (("inside", np.uint8, ()), ("leaf_key", np.uint64, ()), ("leaf_index", np.int32, ()), ("leaf_width", f32, ()),
           ("leaf_center", f32, (3,)), ("target_key", np.uint64, ()))


class Tree(octree_ref.OctTree):
    def __init__(self, center, width):
        super().__init__(center, width, None)

    def contains(self, p, node=None):
        b = self.root if node is None else node
        hw = f32(float(b.w) / 2.0)
        q = [f32(p[k]) for k in range(3)]
        return bool(q[0] > f32(b.c[0] - hw) and q[1] > f32(b.c[1] - hw) and q[2] > f32(b.c[2] - hw) and
                    q[0] <= f32(b.c[0] + hw) and q[1] <= f32(b.c[1] + hw) and q[2] <= f32(b.c[2] + hw))

    def add_at(self, p, e, width):
        """DynOctTree::add(e, width) for an element at p; elements are (p, e) pairs so that a split can re-sort them."""
        leaf = self.at(p)
        while float(leaf.w) / 2.0 > float(f32(width)):
            buf = self.split(leaf)
            for x in buf:
                self.at(x[0], leaf).data.append(x)
            leaf = self.at(p, leaf)
        leaf.data.append((p, e))
        return leaf

    def add_conditional(self, p, e, width):
        """DynOctTree::addConditional: the leaf e went into, or None (the reference returns false and the leaf it found)."""
        width = f32(width)
        leaf = self.at(p)
        if leaf.data or leaf.w < width:
            return None
        while float(leaf.w) / 2.0 > float(width):
            self.split(leaf)
            leaf = self.at(p, leaf)
        leaf.data.append((p, e))
        return leaf

    def key(self, node):
        path = []
        while node is not self.root:
            path.append(node.idx)
            node = node.parent
        k = 1
        for idx in reversed(path):
            k = (k << 3) | idx
        return k

    def node(self, key):
        """The cell with path `key`, making branches on the way."""
        d = (int(key).bit_length() - 1) // 3
        n = self.root
        for lvl in range(d):
            if n.children is None:
                n.make_branch()
            n = n.children[(key >> (3 * (d - 1 - lvl))) & 7]
        return n

    def key_sets(self):
        """(branch keys, {nonempty leaf key: [elements]}, {every leaf key: (centre bytes, width bytes)})."""
        branches, leaves, cells = set(), {}, {}

        def walk(n):
            if n.children is None:
                k = self.key(n)
                cells[k] = (n.c.tobytes(), f32(n.w).tobytes())
                if n.data:
                    leaves[k] = [x[1] for x in n.data]
                return
            if n is not self.root:
                branches.add(self.key(n))
            for ch in n.children:
                walk(ch)

        walk(self.root)
        return branches, leaves, cells


def tree_from_keys(root_center, root_width, branches, leaves):
    """The pointer tree of a key image: leaves {key: element}; an element sits at its leaf's centre."""
    t = Tree(root_center, root_width)
    for k in sorted(branches):
        n = t.node(k)
        if n.children is None:
            n.make_branch()
    for k, e in leaves.items():
        n = t.node(k)
        assert n.children is None
        n.data.append((n.c.copy(), e))
    return t


class Located:
    def __init__(self, n):
        for name, dt, shape in OUTPUTS:
            setattr(self, name, np.zeros((n,) + shape, dt))

    def bytes(self):
        return [getattr(self, name).tobytes() for name, _, _ in OUTPUTS]


class HostOctree:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "liboctree_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.ot_locate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9

    def locate(self, root_center, root_width, branch_key, leaf_key, points, add_width=None):
        """-> (status, verdict bits, Located)"""
        root = np.array(list(root_center[:3]) + [root_width], f32)
        bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
        lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
        pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
        n = len(pts)
        aw = None if add_width is None else np.ascontiguousarray(np.broadcast_to(np.asarray(add_width, f32), (n,)))
        r = Located(n)
        verdict = np.zeros(1, np.int32)
        rc = self.L.ot_locate(root.ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, n, pts.ctypes.data,
                              None if aw is None else aw.ctypes.data, *[getattr(r, name).ctypes.data for name, _, _ in OUTPUTS],
                              verdict.ctypes.data)
        return rc, int(verdict[0]), r


def expand_six(oscene, parents, width, options=None, cache=None, cache_keys=None):
    """The six candidates of every parent before optimize (`pre`) and after it, with the oracle's scale / drift stage (`ref`):
    two oracle.expand_batch calls.  Refinement reads neither the tree nor the maps, so with `cache` (a dict) the candidates of
    parent i are kept under (cache_keys[i], width) and computed once for all the loops that share them."""
    from oracle import oracle as orc
    n = len(parents)
    width = f32(width)
    keys = [None] * n if cache is None else [(cache_keys[i], width.tobytes()) for i in range(n)]
    todo = [i for i in range(n) if cache is None or keys[i] not in cache]
    got = {}
    if todo:
        sub = (orc.Patch * len(todo))(*[parents[i] for i in todo])
        cc, cw = np.zeros((len(todo), 3), f32), np.full(len(todo), width, f32)
        pre = orc.expand_batch(oscene, 0, sub, cc, cw, np.ones(6 * len(todo), np.uint8), options=options, n_threads=8)
        ref = orc.expand_batch(oscene, 0, sub, cc, cw, None, options=options, n_threads=8)
        for j, i in enumerate(todo):
            got[i] = ([pre[6 * j + k] for k in range(6)], [ref[6 * j + k] for k in range(6)])
            if cache is not None:
                cache[keys[i]] = got[i]
    six = [got[i] if i in got else cache[keys[i]] for i in range(n)]
    return [q for a, _ in six for q in a], [q for _, b in six for q in b]


def sequential_extend(oscene, depths, parents, width, tree, margin=1.0, abs_int=0, options=None, events=None, event_cell=(),
                      cache=None, cache_keys=None):
    """CellProcessor::extend over `parents` (an oracle Patch array: the patches of one level's leaves, all of width `width`) in
    order, on the live pointer `tree` (a Tree, or the Tree of a subtree's root) and the live maps `depths`.  Refinement reads
    neither, so oracle.expand_batch refines every candidate up front (expand_six); then candidate by candidate: pre-gate on the tree,
    the oracle's scale / drift stage, OracleDepths.gates, the three thresholds, the border test, addConditional, set_depths.
    events[j] (oracle patches) are subtracted right before the candidates of parent event_cell[j].
    Returns dict(stage, counts, accepted, border, center (refined candidates), tally)."""
    from oracle import oracle as orc
    o = options or orc.default_options()
    n = len(parents)
    N = 6 * n
    width = f32(width)
    pre, ref = expand_six(oscene, parents, width, o, cache, cache_keys)
    stage = np.zeros(N, np.int32)
    counts = np.full((N, 3), -1, np.int32)
    accepted, border = [], []
    tally = dict(pre_shallower_nonempty=0, pre_finer=0, refused=0, border=0, deep_split=0)
    MIN = int(o.MIN_IMAGES_PER_PATCH)
    j = 0
    for t in range(N):
        if t % 6 == 0:
            while events is not None and j < len(events) and event_cell[j] == t // 6:
                depths.set_depths(events[j], subtract=True)
                j += 1
        p = np.array(pre[t].center[:3], f32)
        leaf = tree.at(p)
        if tree.contains(p) and (leaf.data or leaf.w < width):
            stage[t] = 20
            tally["pre_shallower_nonempty"] += bool(leaf.data and leaf.w > width)
            tally["pre_finer"] += bool(leaf.w < width)
            continue
        q = ref[t]
        if q.stage != 0:
            stage[t] = q.stage
            continue
        v, b, f = depths.gates(q, margin, abs_int)
        counts[t] = (v, b, f)
        if not v >= MIN:
            stage[t] = 23
        elif not b < MIN:
            stage[t] = 24
        elif not (f >= MIN - 1 and f * 1.0 / q.n_images > 0.75):
            stage[t] = 25
        else:
            c = np.array(q.center[:3], f32)
            if not tree.contains(c):
                stage[t] = 27
                border.append(t)
                tally["border"] += 1
                continue
            before = tree.depth(tree.at(c))
            new = tree.add_conditional(c, ("extend", t), f32(float(width) * 0.9))
            if new is None:
                stage[t] = 26
                tally["refused"] += 1
                continue
            tally["deep_split"] += tree.depth(new) - before >= 2
            depths.set_depths(q)
            accepted.append(t)
    center = np.array([ref[t].center[:] for t in range(N)], f32).reshape(N, 4)
    normal = np.array([ref[t].normal[:] for t in range(N)], f32).reshape(N, 4)
    return dict(stage=stage, counts=counts, accepted=accepted, border=border, center=center, normal=normal, tally=tally)
