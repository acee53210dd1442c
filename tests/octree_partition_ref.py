"""Test infrastructure for the split into subtrees (hpmvs_octree_partition, frontier.partition):
  * get_sub_trees_loop: the loop of the reference's getSubTrees (src/main.cpp:50-96) as written, on the POINTER tree of
    tests/octree_tree_ref.py -- a recursive nr_leafs (doctree.h:236-247), DynOctTree::getSubTrees over children[0 .. 7]
    (doctree.h:513-523), the list handled exactly as in main -- and what each run shows of the cases the tests must cover;
  * image: its result as the ABI's arrays, read off the pointer tree alone (depth-first walk, Cell objects);
  * HostPartition: hpmvs_amd/csrc/octree.hpp compiled by g++ (tests/octree_partition_host.cpp) into a directory the caller chooses;
  * the trees and parameters the CPU and GPU tests share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import octree_insert_ref as oir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "octree_partition_host.cpp")
f32 = np.float32
MAX_DEPTH = 21
MAX_SUBTREES = 4096
MIN_TREES = (-1, 0, 1, 2, 8, 9, 64, 65, 100, 129, 1000, 4096)
MIN_SPLIT_LEAVES = (1, 3, 100)
OUTPUTS = (("root_key", np.uint64, "cap"), ("root_cell", f32, "cap4"), ("tree_first", np.int32, "cap"), ("tree_leaves", np.int32, "cap"),
           ("leaf_order", np.int32, "nl"), ("leaf_tree", np.int32, "nl"), ("leaf_sub_key", np.uint64, "nl"), ("branch_tree", np.int32, "nb"),
           ("branch_sub_key", np.uint64, "nb"))
CASES = ("a tie decided by list index", "a tie across 64-entry chunks", "a nonempty orphan at depth 1", "a nonempty orphan below a cut subtree",
         "an empty branch that becomes a subtree", "a cut that leaves the list no longer", "a cut that shortens the list", "stop 0", "stop 1",
         "stop 2", "a root at depth 20 with leaves at depth 21")


def capacity(min_trees):
    return max(8, int(min_trees) + 6)


class Arrays:
    """the outputs of hpmvs_octree_partition: info [26] int32 (n_trees, n_orphans, n_splits, stop, histogram [22]) and OUTPUTS"""

    def __init__(self, nb, nl, min_trees, fill=0):
        cap = capacity(min_trees)
        n = dict(cap=(cap,), cap4=(cap, 4), nl=(nl,), nb=(nb,))
        self.info = np.zeros(26, np.int32)
        for name, dt, shape in OUTPUTS:
            a = np.zeros(n[shape], dt)
            a.view(np.uint8)[...] = fill
            setattr(self, name, a)

    def bytes(self):
        return [self.info.tobytes()] + [getattr(self, name).tobytes() for name, _, _ in OUTPUTS]

    def differences(self, other):
        return [name for name, a, b in zip(("info",) + tuple(o[0] for o in OUTPUTS), self.bytes(), other.bytes()) if a != b]


class HostPartition:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "liboctree_partition_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.ot_partition.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10

    def partition(self, root_center, root_width, branch_key, leaf_key, min_trees, min_split_leaves, fill=0):
        """-> (status, Arrays)"""
        root = np.array(list(root_center[:3]) + [root_width], f32)
        bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
        lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
        r = Arrays(len(bk), len(lk), min_trees, fill)
        if fill:
            r.info.view(np.uint8)[...] = fill
        rc = self.L.ot_partition(root.ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, int(min_trees), int(min_split_leaves),
                                 r.info.ctypes.data, *[getattr(r, name).ctypes.data for name, _, _ in OUTPUTS])
        return rc, r


# ---- trees: (root centre, root width, branch keys, nonempty leaf keys), the key arrays permuted

def grown_tree(seed, n_leaves, max_depth=6, spare=2.0):
    """cells split at random until there are `spare` times n_leaves leaf cells, n_leaves of them nonempty: exactly n_leaves
    leaves, empty leaves beside them and branches with nothing below"""
    rng = np.random.default_rng(seed)
    cells, branches = [(1 << 3) | i for i in range(8)], []
    while len(cells) < spare * n_leaves:
        j = int(rng.integers(len(cells)))
        if oir.key_depth(cells[j]) >= max_depth:
            continue
        k = cells.pop(j)
        branches.append(k)
        cells += [(k << 3) | i for i in range(8)]
    leaves = [cells[i] for i in rng.permutation(len(cells))[:n_leaves]]
    return (np.array([0.25, -0.5, 1.0], f32), f32(3.0), rng.permutation(np.array(branches, np.uint64)), rng.permutation(np.array(leaves, np.uint64)))


def crafted_tree():
    """depth 1: child 0 a nonempty leaf (an orphan), 1 a branch with nothing below, 2 and 5 branches with three leaves each (a
    tie), 3 a branch whose only content is ONE branch with eight leaves (its cut leaves the list no longer; the cut of that one
    shortens it), 6 a branch with a leaf child and a branch child of four leaves (an orphan below a cut)"""
    b, l = [0o11, 0o12, 0o15, 0o13, 0o134, 0o16, 0o167], [0o10]
    l += [0o120, 0o123, 0o127, 0o151, 0o152, 0o156]
    l += [0o1340 + i for i in range(8)]
    l += [0o162] + [0o1670 + i for i in (1, 2, 4, 7)]
    rng = np.random.default_rng(3)
    return np.array([0, 0, 0], f32), f32(2.0), rng.permutation(np.array(b, np.uint64)), rng.permutation(np.array(l, np.uint64))


def deep_tree():
    """a chain of branches down to depth 19 whose last has two branch children, each with three leaves at depth 21"""
    key, b = 1, []
    for d in range(19):
        key = (key << 3) | (d * 5 % 8)
        b.append(key)
    pair = [(key << 3) | 2, (key << 3) | 6]
    l = [(p << 3) | i for p in pair for i in (0, 3, 7)]
    rng = np.random.default_rng(4)
    return np.array([1, 1, 1], f32), f32(64.0), rng.permutation(np.array(b + pair, np.uint64)), rng.permutation(np.array(l, np.uint64))


def _permuted(name):
    center, W, bk, lk = oir.TREES[name]()
    rng = np.random.default_rng(len(bk))
    return center, W, rng.permutation(bk), rng.permutation(lk)


TREES = {"empty": oir.empty_tree, "chain": functools.partial(_permuted, "chain"), "random": functools.partial(_permuted, "random"),
         "crafted": crafted_tree, "deep": deep_tree, "grown-700": functools.partial(grown_tree, 700, 700, 5, 1.3)}
EDGE_LEAVES = (63, 64, 65, 255, 256, 257)        # key counts on wave and block edges


@functools.lru_cache(maxsize=None)
def tree(name):
    return TREES[name]() if name in TREES else grown_tree(int(name), int(name))


# ---- the reference loop

@functools.lru_cache(maxsize=None)
def pointer_tree(name):
    center, W, bk, lk = tree(name)
    return oir.pointer_tree(center, W, bk, lk)


def nr_leafs(node, memo=None):
    """Branch::nrLeafs (doctree.h:236-247), "recursive and slow!"; memo: id(node) -> count, for a tree that does not change"""
    if memo is not None and id(node) in memo:
        return memo[id(node)]
    leafs = 0
    for ch in node.children:
        if ch.children is None and ch.data:
            leafs += 1
        elif ch.children is not None:
            leafs += nr_leafs(ch, memo)
    if memo is not None:
        memo[id(node)] = leafs
    return leafs


def get_sub_trees(node):
    """DynOctTree::getSubTrees (doctree.h:513-523): the BRANCH children in child order; the empty() test is commented out"""
    return [ch for ch in node.children if ch.children is not None]


def get_sub_trees_loop(T, min_trees, min_split_leaves=100, memo=None):
    """main.cpp:50-96 on the pointer tree T -> dict(trees: the list of subtree roots (Cell objects), n_splits, stop, shown: the
    set of CASES this run shows).  memo: nr_leafs' counts, which runs on one unchanged tree may share."""
    memo, shown = {} if memo is None else memo, set()
    if min_trees < 2:
        return dict(trees=[T.root], n_splits=0, stop=0, shown={"stop 0"})
    sub = get_sub_trees(T.root)
    if any(ch.children is None and ch.data for ch in T.root.children):
        shown.add(CASES[2])
    n_splits, stop = 0, 1
    counts = [nr_leafs(n, memo) for n in sub]                # main recomputes them in every iteration: the tree does not change
    while len(sub) < min_trees:
        # "if (nrLeafs > maxLeafs)" from maxLeafs = -1 over ii = 0 ..: the first entry with the largest count
        max_leafs = max(counts, default=-1)
        max_index = counts.index(max_leafs) if counts else -1
        if max_leafs < min_split_leaves:
            stop = 2
            break
        if counts.count(max_leafs) > 1:
            shown.add(CASES[0])
            last = len(counts) - 1 - counts[::-1].index(max_leafs)
            if last // 64 != max_index // 64:
                shown.add(CASES[1])
        max_tree = sub[max_index]
        if any(ch.children is None and ch.data for ch in max_tree.children):
            shown.add(CASES[3])
        new = get_sub_trees(max_tree)
        shown.add(CASES[5] if len(new) == 1 else CASES[6] if len(new) == 0 else "")
        counts = [nr_leafs(n, memo) for n in new] + counts[:max_index] + counts[max_index + 1:]
        sub = new + sub[:max_index] + sub[max_index + 1:]    # "for ii: if (ii != maxIndex) newSubTrees.push_back(subTrees[ii])"
        n_splits += 1
    shown.add("stop %d" % stop)
    for n in sub:
        if nr_leafs(n, memo) == 0:
            shown.add(CASES[4])
        if T.depth(n) == 20 and any(ch.data for ch in n.children):
            shown.add(CASES[10])
    shown.discard("")
    return dict(trees=sub, n_splits=n_splits, stop=stop, shown=shown)


_counts = {}


@functools.lru_cache(maxsize=None)
def loop(name, min_trees, min_split_leaves):
    """get_sub_trees_loop on pointer_tree(name), once for all the tests that read it"""
    return get_sub_trees_loop(pointer_tree(name), min_trees, min_split_leaves, _counts.setdefault(name, {}))


def image(T, bk, lk, min_trees, result):
    """The loop's result as the ABI's arrays (Arrays), by one depth-first walk of the pointer tree (children 0 .. 7: Leaf_iterator
    order); elements of T are ("seed", index into lk) as oir.pointer_tree makes them."""
    r = Arrays(len(bk), len(lk), min_trees)
    index = {id(n): t for t, n in enumerate(result["trees"])}
    branch_at = {int(k): j for j, k in enumerate(bk)}
    n_trees = len(index)
    order, held = [], 0

    def walk(node, key, depth, owner, sub):
        nonlocal held
        t = index.get(id(node), -1)
        if t >= 0:
            assert owner < 0, "nested roots"
            r.root_key[t], r.tree_first[t], r.tree_leaves[t] = key, len(order), nr_leafs(node)
            r.root_cell[t, :3], r.root_cell[t, 3] = node.c, node.w
            held += int(r.tree_leaves[t])
        if node.children is None:
            if node.data:
                j = node.data[0][1][1]
                assert int(lk[j]) == key
                r.leaf_tree[j], r.leaf_sub_key[j] = owner, sub
                r.info[4 + depth] += 1
                order.append(j)
            return
        if depth > 0:
            j = branch_at[key]
            r.branch_tree[j], r.branch_sub_key[j] = owner, sub
        for i, ch in enumerate(node.children):
            if ch.children is None and not ch.data:            # an empty leaf: in no output
                continue
            if t >= 0:
                walk(ch, (key << 3) | i, depth + 1, t, (1 << 3) | i)
            else:
                walk(ch, (key << 3) | i, depth + 1, owner, (sub << 3) | i if owner >= 0 else 0)

    walk(T.root, 1, 0, -1, 0)
    r.leaf_order[:] = order
    r.info[:4] = n_trees, len(lk) - held, result["n_splits"], result["stop"]
    return r
