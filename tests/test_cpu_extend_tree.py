"""The extend level's two octree look-ups, host side.  The g++ build of hpmvs_amd/csrc/octree.hpp's extend_pre / extend_post /
level_depth (tests/extend_tree_host.cpp) equals, byte for byte, a restatement of the reference's lines on the pointer tree of
tests/octree_tree_ref.py: CellProcessor.cpp:122-125 (the pre-gate: inside the root, in a leaf that is nonempty or narrower than the
cell), :147-154 (the border test, then addConditional at width * 0.9) and doctree.h:397-419 (addConditional).  Trees: the random
trees of test_cpu_octree_index.py and the empty tree; points: random, on split planes, on root faces, outside, NaN / inf; widths:
every level width of the tree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import octree_tree_ref as otr
from test_cpu_octree_index import _random_tree, _special_points

f32 = np.float32
SRC = os.path.join(otr.ROOT, "tests", "extend_tree_host.cpp")
HPMVS_ERR_ARG = -2
CASES = ("skip_shallower_nonempty", "skip_finer", "refused_inside", "border", "outside_pre", "deep_target")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("extend_tree_host")), "libextend_tree_host.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
    L = C.CDLL(so)
    L.et_level_depth.argtypes = [C.c_float, C.c_float]
    L.et_add_width.argtypes = [C.c_float]
    L.et_add_width.restype = C.c_float
    L.et_extend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 5
    return L


def _level_widths(W):
    """width_ of the cells of depth 0 .. 21: Cell(parent, idx) halves in double and stores a float."""
    w = [f32(W)]
    for _ in range(otr.MAX_DEPTH):
        w.append(f32(float(w[-1]) / 2.0))
    return w


def _reference(T, points, width, tally):
    """Per point (skip, pre_inside, pre_key, border, post_key) from the reference's lines on the pointer tree T."""
    width = f32(width)
    add_width = f32(float(width) * 0.9)                       # cell->width_ * 0.9 through addConditional's float parameter
    n = len(points)
    skip, inside, border = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    pre_key, post_key = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for i, p in enumerate(points):
        leaf = T.at(p)
        inside[i] = T.contains(p)                             # getRoot()->contains
        border[i] = not inside[i]                             # :147
        tally["outside_pre"] += not inside[i]
        tally["border"] += not inside[i]
        if not inside[i]:
            continue
        skip[i] = bool(leaf.data) or bool(leaf.w < width)     # :124
        tally["skip_shallower_nonempty"] += bool(leaf.data) and bool(leaf.w > width)
        tally["skip_finer"] += bool(leaf.w < width)
        before = T.depth(leaf)
        new = T.add_conditional(p, "probe", add_width)        # :150, doctree.h:397-419
        pre_key[i] = post_key[i] = 0 if new is None else T.key(new)
        tally["refused_inside"] += new is None
        tally["deep_target"] += new is not None and T.depth(new) - before >= 2
        leaf.children, leaf.data = None, ([] if new is not None else leaf.data)     # undo the probe's splits
    return skip, inside, pre_key, border, post_key


def _host(L, center, W, bk, lk, points, width):
    root = np.array(list(center[:3]) + [W], f32)
    n = len(points)
    pts = np.ascontiguousarray(points, f32).reshape(n, 3)
    out = [np.full(n, 0x5A, np.uint8), np.full(n, 0x5A, np.uint8), np.full(n, 0x5A5A, np.uint64), np.full(n, 0x5A, np.uint8),
           np.full(n, 0x5A5A, np.uint64)]
    rc = L.et_extend(root.ctypes.data, len(bk), bk.ctypes.data, len(lk), lk.ctypes.data, n, pts.ctypes.data, float(width),
                     *[a.ctypes.data for a in out])
    return rc, out


def _trees():
    rng = np.random.default_rng(7)
    for what, n_leaves, deep in (("random", 400, False), ("deep", 120, True)):
        T, center, W, pts = _random_tree(rng, n_leaves, deep=deep)
        yield what, T, center, W, _special_points(rng, T, center, W, pts)
    center, W = np.array([1, 2, 3], f32), f32(4.0)
    T = otr.Tree(center, W)
    yield "empty", T, center, W, _special_points(rng, T, center, W, (center + rng.uniform(-0.5, 0.5, (100, 3)) * 4).astype(f32))


def test_extend_pre_and_post_equal_the_reference_lines_on_the_pointer_tree(host):
    total = dict.fromkeys(CASES, 0)
    work = []
    for what, T, center, W, points in _trees():
        branches, leaves, _ = T.key_sets()
        bk, lk = np.array(sorted(branches), np.uint64), np.array(sorted(leaves), np.uint64)
        odd = points[-12:]                                    # NaN / inf: at every width
        for d, width in enumerate(_level_widths(W)[1:], 1):
            # every eighth point per width, the phase moving with the depth: each kind of point meets each width
            pts = np.concatenate([points[:-12][(d - 1) % 8::8], odd])
            tally = dict.fromkeys(CASES, 0)
            want = _reference(T, pts, width, tally)
            for k in CASES:
                total[k] += tally[k]
            work.append((what, d, center, W, bk, lk, pts, width, want))
    # the inputs first, on the restatement alone: every fate occurs
    assert min(total.values()) >= 1, total
    for what, d, center, W, bk, lk, pts, width, want in work:
        assert host.et_level_depth(float(W), float(width)) == d, (what, d)
        assert f32(host.et_add_width(float(width))).tobytes() == f32(float(width) * 0.9).tobytes(), (what, d)
        rc, got = _host(host, center, W, bk, lk, pts, width)
        assert rc == 0, (what, d)
        for name, a, b in zip(("skip", "pre_inside", "pre_key", "border", "post_key"), got, want):
            assert a.tobytes() == b.tobytes(), (what, d, name, np.nonzero(a != b)[0][:5])
    # the tree alone decides: an empty tree pre-gates nothing and refuses nothing
    assert total["skip_finer"] and total["refused_inside"]


def test_level_depth_accepts_the_level_widths_only(host):
    for W in (f32(7.0), f32(4.0), f32(0.3), f32(1e-3), f32(12345.678)):
        widths = _level_widths(W)
        for d in range(1, otr.MAX_DEPTH + 1):
            w = widths[d]
            assert host.et_level_depth(float(W), float(w)) == d
            for bad in (np.nextafter(w, f32(np.inf)), np.nextafter(w, f32(0)), f32(float(w) * 0.9)):
                assert host.et_level_depth(float(W), float(bad)) == -1, (W, d, bad)
        for bad in (W, f32(0), f32(np.nan), f32(np.inf), f32(-np.inf), -widths[3], f32(float(widths[otr.MAX_DEPTH]) / 2.0)):
            assert host.et_level_depth(float(W), float(bad)) == -1, (W, bad)


def test_a_width_that_is_no_level_width_writes_nothing(host):
    center, W = np.zeros(3, f32), f32(2.0)
    none = np.zeros(0, np.uint64)
    rc, out = _host(host, center, W, none, none, np.zeros((4, 3), f32), f32(0.9))
    assert rc == HPMVS_ERR_ARG and all((a == a.dtype.type(0x5A5A if a.dtype == np.uint64 else 0x5A)).all() for a in out)
