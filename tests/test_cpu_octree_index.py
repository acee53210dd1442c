"""The real octree as path keys, host side.  frontier.Octree (branch-key set + leaf dict) equals the pointer tree of
tests/octree_tree_ref.py after random sequences of add(width), addConditional, split and remove -- leaf paths, width and centre
bits, data, the branch set -- and the g++ build of hpmvs_amd/csrc/octree.hpp (tests/octree_host.cpp) equals the pointer tree's
at(), contains() and addConditional's target exactly, on points that sit on split planes and root faces, outside the root, at
NaN / +-inf, and in the empty tree."""
import numpy as np
import pytest

import octree_tree_ref as otr
import seed_tree_ref as sr

f32 = np.float32
HPMVS_ERR_ARG = -2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return otr.HostOctree(tmp_path_factory.mktemp("octree_host"))


def _octree(center, width):
    from hpmvs_amd import frontier
    return frontier.Octree(center, width)


def _assert_same(T, O, what=""):
    branches, leaves, cells = T.key_sets()
    assert branches == O.branches, (what, sorted(branches ^ O.branches)[:5])
    assert {k: [x[1] for x in row] for k, row in O.leaves.items()} == leaves, what
    for k, (c, w) in cells.items():   # every leaf, empty ones included
        oc, ow = O.cell(k)
        assert oc.tobytes() == c and f32(ow).tobytes() == w, (what, hex(k))
        assert k not in O.branches and ((k >> 3) == 1 or (k >> 3) in O.branches), (what, hex(k))
    keys, rows, cc, cw = O.leaf_table()
    order = [T.key(l) for l in T.nonempty()]          # Leaf_iterator order
    assert keys.tolist() == order, what
    assert cc.tobytes() == b"".join(cells[k][0] for k in order) and cw.tobytes() == b"".join(cells[k][1] for k in order), what


def _add(O, p, e, width):
    """DynOctTree::add through the Octree's own operations."""
    key = O.at(p)
    while float(O.cell(key)[1]) / 2.0 > float(f32(width)):
        row = O.split(key) or []
        for x in row:
            ch = O.at(x[0], key)
            if ch in O.leaves:
                O.leaves[ch].append(x)
            else:
                O.insert(ch, [x])
        key = O.at(p, key)
    if key in O.leaves:
        O.leaves[key].append((p, e))
    else:
        O.insert(key, [(p, e)])
    return key


@pytest.mark.parametrize("seed", [1, 2])
def test_octree_equals_the_pointer_tree_under_random_operations(seed):
    rng = np.random.default_rng(seed)
    n = 500
    pts = rng.normal(0, 1, (n, 3)).astype(f32)
    pts[:50] = pts[50:100] + rng.normal(0, 1e-5, (50, 3)).astype(f32)     # near-coincident pairs: deep splits
    center, W = np.array([0.1, -0.2, 0.05], f32), f32(9.0)
    T, O = otr.Tree(center, W), _octree(center, W)
    deepest, collapsed, refused, ops = 0, 0, 0, 0
    for step in range(2000):
        kind = rng.choice(["add", "cond", "split", "remove"], p=[0.35, 0.3, 0.1, 0.25])
        i = int(rng.integers(n))
        p = pts[i]
        width = f32(float(W) * 2.0 ** -(int(rng.integers(1, 22)) + 0.5))
        if kind == "add":
            leaf = T.add_at(p, step, width)
            assert _add(O, p, step, width) == T.key(leaf)
        elif kind == "cond":
            leaf = T.add_conditional(p, step, width)
            key = O.add_conditional(p, width, [(p, step)])
            assert (key is None) == (leaf is None) and (leaf is None or key == T.key(leaf))
            refused += leaf is None
        elif kind == "split":
            leaf = T.at(p)
            if T.depth(leaf) >= 21:
                continue
            data = T.split(leaf)
            row = O.split(T.key(leaf))
            assert [x[1] for x in (row or [])] == [x[1] for x in data]
        else:
            leaf = T.at(p)
            key = T.key(leaf)
            after = T.remove(leaf)
            assert O.remove(key) == T.key(after)
            collapsed += after is not leaf
        ops += 1
        deepest = max(deepest, max((int(k).bit_length() - 1) // 3 for k in O.leaves) if O.leaves else 0)
        if step % 100 == 99:
            _assert_same(T, O, f"step {step}")
    _assert_same(T, O, "end")
    assert ops >= 1900 and deepest == 21 and collapsed >= 20 and refused >= 50, (ops, deepest, collapsed, refused)


def test_remove_collapses_one_level_and_leaves_the_empty_grandparent():
    center, W = np.zeros(3, f32), f32(8.0)
    T, O = otr.Tree(center, W), _octree(center, W)
    p = np.array([0.3, 0.3, 0.3], f32)
    leaf = T.add_conditional(p, 0, f32(0.9))                  # depth 3: width 1
    key = O.add_conditional(p, f32(0.9), [(p, 0)])
    assert key == T.key(leaf) and (int(key).bit_length() - 1) // 3 == 3
    after = T.remove(leaf)
    assert O.remove(key) == T.key(after) == key >> 3          # the parent became one empty leaf ...
    assert O.branches == {key >> 6} and not O.leaves          # ... and the grandparent stays a Branch of eight empty leaves
    _assert_same(T, O)
    assert O.at(p) == key >> 3
    # removing in that leaf again: the grandparent's subtree is empty now, so it collapses in turn; the root never does
    assert O.remove(key >> 3) == T.key(T.remove(T.at(p))) == key >> 6
    assert not O.branches
    assert O.remove(key >> 6) == T.key(T.remove(T.at(p))) == key >> 6
    _assert_same(T, O)


def _random_tree(rng, n_leaves, W=f32(7.0), deep=False):
    center = np.array([0.5, -1.0, 2.0], f32)
    T = otr.Tree(center, W)
    pts = (rng.uniform(-0.5, 0.5, (n_leaves, 3)) * float(W) + center).astype(f32)
    for i, p in enumerate(pts):
        T.add_at(p, i, f32(float(W) * 2.0 ** -rng.uniform(2, 21 if deep else 9)))
    for i in rng.integers(0, n_leaves, n_leaves // 10):       # empty structure: finer than anything around it
        leaf = T.at(pts[i])
        T.remove(leaf)
    return T, center, W, pts


def _special_points(rng, T, center, W, pts):
    hw = f32(float(W) / 2.0)
    out = [pts, (pts + rng.normal(0, 0.01, pts.shape)).astype(f32), (center + rng.uniform(-1.5, 1.5, (300, 3)) * float(W)).astype(f32)]
    nodes = []

    def walk(n):
        nodes.append(n)
        if n.children is not None and len(nodes) < 4000:
            for ch in n.children:
                walk(ch)

    walk(T.root)
    planes = []
    for n in [nodes[i] for i in rng.integers(0, len(nodes), 400)]:        # on a split plane in one, two or three axes
        p = (n.c + rng.uniform(-0.5, 0.5, 3) * float(n.w)).astype(f32)
        axes = rng.random(3) < 0.5
        p[axes] = n.c[axes]
        planes.append(p)
        planes.append(np.nextafter(p, f32(np.inf)).astype(f32))
    out.append(np.array(planes, f32))
    faces = []
    for k in range(3):                                                     # the root's faces: > below, <= above
        for face in (f32(center[k] - hw), f32(center[k] + hw)):
            for side in (face, np.nextafter(face, f32(-np.inf)), np.nextafter(face, f32(np.inf))):
                p = (center + rng.uniform(-0.4, 0.4, 3) * float(W)).astype(f32)
                p[k] = side
                faces.append(p)
    out.append(np.array(faces, f32))
    odd = np.tile(center, (12, 1)).astype(f32)
    for r, (k, v) in enumerate([(0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (1, -np.inf), (2, np.inf)]):
        odd[r, k] = v
    odd[6] = np.nan
    odd[7] = [np.inf, -np.inf, np.nan]
    odd[8:] += f32(0.3)
    odd[8, 0], odd[9, 1], odd[10, 2], odd[11, 0] = np.nan, np.inf, -np.inf, -0.0
    out.append(odd)
    return np.concatenate(out).astype(f32)


def _check_against_tree(host, T, center, W, points, widths, what):
    branches, leaves, _ = T.key_sets()
    bk = np.array(sorted(branches), np.uint64)
    lk = np.array(sorted(leaves), np.uint64)
    index = {int(k): i for i, k in enumerate(lk)}
    rc, verdict, r = host.locate(center, W, bk, lk, points, widths)
    assert rc == 0 and verdict == 0, what
    tallies = dict(outside=0, nonempty=0, refused_finer=0, split=0)
    for i, p in enumerate(points):
        leaf = T.at(p)
        key = T.key(leaf)
        assert int(r.leaf_key[i]) == key, (what, i, p)
        assert int(r.leaf_index[i]) == index.get(key, -1), (what, i)
        assert r.leaf_width[i].tobytes() == f32(leaf.w).tobytes() and r.leaf_center[i].tobytes() == leaf.c.tobytes(), (what, i)
        assert bool(r.inside[i]) == T.contains(p), (what, i, p)
        new = T.add_conditional(p, "probe", widths[i])
        assert int(r.target_key[i]) == (0 if new is None else T.key(new)), (what, i, p, widths[i])
        tallies["outside"] += not T.contains(p)
        tallies["nonempty"] += key in index
        tallies["refused_finer"] += new is None and key not in index
        tallies["split"] += new is not None and new is not leaf
        leaf.children, leaf.data = None, ([] if new is not None else leaf.data)     # undo the probe's splits
    return tallies, r


def test_host_restatement_equals_the_pointer_tree(host):
    rng = np.random.default_rng(7)
    for what, n_leaves, deep in (("random", 400, False), ("deep", 120, True)):
        T, center, W, pts = _random_tree(rng, n_leaves, deep=deep)
        points = _special_points(rng, T, center, W, pts)
        widths = (float(W) * 2.0 ** -rng.uniform(0, 20 if deep else 10, len(points))).astype(f32)
        widths[::7] = (float(W) * 2.0 ** -rng.integers(1, 12, len(widths[::7]))).astype(f32)      # exact level widths
        tallies, _ = _check_against_tree(host, T, center, W, points, widths, what)
        assert min(tallies.values()) >= 20, (what, tallies)


def test_host_restatement_on_the_empty_tree(host):
    center, W = np.array([1, 2, 3], f32), f32(4.0)
    T = otr.Tree(center, W)
    rng = np.random.default_rng(3)
    points = _special_points(rng, T, center, W, (center + rng.uniform(-0.5, 0.5, (100, 3)) * 4).astype(f32))
    widths = (4.0 * 2.0 ** -rng.uniform(0, 20, len(points))).astype(f32)
    tallies, r = _check_against_tree(host, T, center, W, points, widths, "empty")
    assert (r.leaf_index == -1).all() and (r.leaf_width == f32(2.0)).all() and ((r.leaf_key >= 8) & (r.leaf_key < 16)).all()
    # without add_width: no target keys
    rc, _, r2 = host.locate(center, W, [], [], points, None)
    assert rc == 0 and not r2.target_key.any() and r2.leaf_key.tobytes() == r.leaf_key.tobytes()


def test_malformed_tables_are_refused(host):
    c, W = np.zeros(3, f32), f32(2.0)
    p = np.zeros((1, 3), f32)
    deep21 = (1 << 63) | 5
    cases = {
        "orphan leaf": ([], [0o112]), "orphan branch": ([0o112], []), "branch and leaf": ([0o11], [0o11]),
        "duplicate leaf": ([], [0o11, 0o11]), "duplicate branch": ([0o11, 0o11], []), "zero": ([], [0]), "the root": ([1], []),
        "off-grid sentinel": ([], [0o21]), "branch at depth 21": ([deep21], []),
    }
    for what, (bk, lk) in cases.items():
        rc, verdict, r = host.locate(c, W, bk, lk, p, None)
        assert rc == HPMVS_ERR_ARG and verdict and not r.leaf_key.any(), what
    chain = [(1 << (3 * d)) | 0 for d in range(1, 21)]                       # a 21-level chain is a tree
    rc, verdict, r = host.locate(c, W, chain, [1 << 63], np.full((1, 3), -1.0, f32), None)
    assert rc == 0 and int(r.leaf_key[0]) == 1 << 63 and r.leaf_index[0] == 0


def test_subtree_is_the_tree_below_its_root():
    rng = np.random.default_rng(11)
    T, center, W, pts = _random_tree(rng, 300)
    branches, leaves, _ = T.key_sets()
    O = _octree(center, W)
    O.branches = set(branches)
    for k, e in leaves.items():
        O.insert(k, e)
    root = max((k for k in branches if (int(k).bit_length() - 1) // 3 == 2), key=lambda k: sum(1 for l in leaves if l >> (3 * ((int(l).bit_length() - 1) // 3 - 2)) == k))
    S = O.subtree(root)
    assert S.root_level == 2 and S.root_center.tobytes() == O.cell(root)[0].tobytes() and S.root_width == O.cell(root)[1]
    inside = 0
    for p in pts:
        full = O.at(p)
        d = (int(full).bit_length() - 1) // 3
        if d > 2 and full >> (3 * (d - 2)) == root:
            inside += 1
            sub = S.at(p)
            assert S.contains(p)
            assert sub == (full & ((1 << (3 * (d - 2))) - 1)) | (1 << (3 * (d - 2)))
            assert S.row(sub) == O.row(full) and S.node_level(sub) == O.node_level(full)
            assert S.cell(sub)[0].tobytes() == O.cell(full)[0].tobytes() and S.cell(sub)[1] == O.cell(full)[1]
    assert inside >= 10 and len(S.leaves) >= 5


def test_from_seed_tree_gives_the_sequential_insertion():
    from hpmvs_amd import frontier
    name, center, scale, ok, maxlevel = sr.clouds()[0]
    ref = sr.sequential(center[:400], scale[:400], None, maxlevel)
    L = ref["leaves"]
    st = frontier.SeedTree(ref["root_center"], float(ref["root_width"]), float(ref["scale_floor"]), np.zeros(0, np.int32),
                           np.zeros(len(L) + 1, np.int32), np.array([l[1] for l in L], f32), np.array([l[2] for l in L], f32),
                           np.array([l[3] for l in L], np.int32), np.zeros((len(L), 3), f32))
    O = frontier.Octree.from_seed_tree(st)
    want = {(1 << (3 * l[3])) | (l[0] >> (3 * (21 - l[3]))): i for i, l in enumerate(L)}
    assert O.leaves == want
    assert O.branches == {k >> (3 * j) for k in want for j in range(1, (int(k).bit_length() - 1) // 3)}
    assert len({l[3] for l in L}) >= 3                                     # leaves on several levels
    keys, rows, cc, cw = O.leaf_table()
    assert rows == list(range(len(L)))                                     # Leaf_iterator order is the seed tree's
