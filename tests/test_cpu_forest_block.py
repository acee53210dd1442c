"""The forest's device block, host side: hpmvs_amd/csrc/octree.hpp's forest_block / forest_block_fill, which lay out and fill what
hpmvs_extend_forest_batch, hpmvs_process_forest_batch and hpmvs_border_forest_batch upload.  tests/forest_block_host.cpp holds
the checks (fb_check returns the line of the first one that fails): every offset a multiple of 256, the regions in order and
apart, end behind the values, slots as forest_slots counts them; in the header filled for a made-up device address the verdict
words good, the offset arrays verbatim, every Tree with its root and its slot range of the keys and the values; and
forest_build_sequential over a block laid out this way giving the verdict and the tables it gives over plain vectors.  Here: the
forests it must hold for, each with no extra header bytes and with n_trees of them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("forest_block_host")), "libforest_block_host.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "forest_block_host.cpp"),
                    "-o", so], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.fb_check.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_size_t]
    return lib


def _tree(rng, n_leaves):
    """(branch keys, leaf keys): distinct leaves at depth 2 and the depth-1 branches above them, shuffled"""
    cells = rng.choice(64, n_leaves, replace=False)
    lk = (0o100 | cells).astype(np.uint64)
    bk = (0o10 | np.unique(cells >> 3)).astype(np.uint64)
    rng.shuffle(bk)
    return bk, lk


def _forests():
    rng = np.random.default_rng(21)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    one_leaf = (np.zeros(0, np.uint64), np.array([0o13], np.uint64))
    many = [_tree(rng, int(rng.integers(0, 33))) for _ in range(130)]        # 0-40 keys each: up to 32 leaves under up to 8 branches
    assert min(len(b) + len(l) for b, l in many) == 0 and 30 < max(len(b) + len(l) for b, l in many) <= 40
    return {"no tree": [], "one tree without keys": [none], "one tree with one leaf key": [one_leaf],
            "three trees, the middle one without keys": [_tree(rng, 20), none, _tree(rng, 7)], "130 trees": many}


@pytest.mark.parametrize("name", list(_forests()))
def test_block_layout_header_and_build(host, name):
    trees = _forests()[name]
    T = len(trees)
    rng = np.random.default_rng(22)
    roots = np.ascontiguousarray(rng.uniform(-50, 50, (T, 4)), np.float32)
    roots[:, 3] = 2.0 ** rng.integers(0, 4, T)
    first = lambda which: np.concatenate([[0], np.cumsum([len(t[which]) for t in trees])]).astype(np.int32)
    bf, lf = first(0), first(1)
    bk = np.concatenate([t[0] for t in trees] + [np.zeros(0, np.uint64)])
    lk = np.concatenate([t[1] for t in trees] + [np.zeros(0, np.uint64)])
    for extra in (0, T):
        line = host.fb_check(T, roots.ctypes.data, bf.ctypes.data, lf.ctypes.data, bk.ctypes.data, lk.ctypes.data, extra)
        assert line == 0, f"{name}, {extra} extra bytes: the check at tests/forest_block_host.cpp:{line} failed"
