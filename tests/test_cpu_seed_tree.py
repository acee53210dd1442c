"""The seed octree's closed form, host side: hpmvs_amd/csrc/seed_tree.hpp compiled by g++ (tests/seed_tree_host.cpp: bounding box,
root, floor, depths, keys, sort, clamp scans, sort, run heads) equals the sequential DynOctTree::add of tests/octree_ref.py from
a root built with the reference's bounding-box fold -- root, floored scales, leaf paths, centres, widths, levels, leaf order and
data order, bit for bit (root_center with ==: the sign of a zero extreme depends on insertion order)."""
import numpy as np
import pytest

import seed_tree_ref as sr

HPMVS_ERR_ARG = -2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sr.HostSeedTree(tmp_path_factory.mktemp("seed_tree_host"))


CLOUDS = sr.clouds()


def test_clouds_cover_the_cases():
    names = [c[0] for c in CLOUDS]
    assert len(set(names)) == len(names)
    assert {c[4] for c in CLOUDS} >= {0, 9, 20}
    by = {c[0]: c for c in CLOUDS}
    assert (by["all-negative"][1][:, :3] < 0).all()
    assert np.isnan(by["nan-and-ok"][1]).any() and np.isnan(by["nan-and-ok"][2]).any()
    assert len(by["zero"][2]) == 0 and len(by["one"][2]) == 1


@pytest.mark.parametrize("cloud", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_host_restatement_equals_sequential_insertion(host, cloud):
    name, center, scale, ok, maxlevel = cloud
    rc, res = host.tree(center, scale, ok, maxlevel)
    assert rc == 0
    ref = sr.assert_equals_sequential(res, center, scale, ok, maxlevel, name)
    if name == "zero" or name == "none-ok":   # the reference's unit cube
        assert res.info[0]["root_center"].tolist() == [0, 0, 0] and res.info[0]["root_width"] == 2 and res.info[0]["n_leaves"] == 0
    if name == "maxlevel-20":
        assert max(leaf[3] for leaf in ref["leaves"]) == 20
    if name == "all-negative":   # max stays at FLT_MIN: the root reaches up to 0
        assert np.all(res.info[0]["root_center"] + res.info[0]["root_width"] / 2 >= 0)


def test_permuted_rows_give_the_same_leaves_in_row_order(host):
    _, center, scale, _, maxlevel = CLOUDS[1]   # coincident centres: leaves with many elements
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(scale))
    rc, a = host.tree(center, scale, None, maxlevel)
    rc2, b = host.tree(center[perm], scale[perm], None, maxlevel)
    assert rc == 0 and rc2 == 0
    sr.assert_equals_sequential(b, center[perm], scale[perm], None, maxlevel, "permuted")
    L = int(a.info[0]["n_leaves"])
    assert int(b.info[0]["n_leaves"]) == L
    assert a.leaf_key[:L].tolist() == b.leaf_key[:L].tolist() and sr.same_bits(a.cell_center, b.cell_center)
    multi = 0
    for l in range(L):
        ra = a.rows[a.cell_start[l]:a.cell_start[l + 1]]
        rb = b.rows[b.cell_start[l]:b.cell_start[l + 1]]
        assert sorted(perm[rb].tolist()) == ra.tolist()   # the same elements ...
        assert rb.tolist() == sorted(rb.tolist())          # ... in the order of the rows they now have
        multi += len(ra) > 1
    assert multi > 10


def test_clamp_composition_is_associative(host):
    rng = np.random.default_rng(11)
    for _ in range(2000):
        t = []
        for _ in range(3):
            lo, hi = sorted(rng.integers(0, 24, 2).tolist())
            t.append((lo, hi))
        x, y = host.clamp_assoc(*t)
        assert x == y, t


def test_depth_alone_is_the_literal_halving_loop(host):
    for rw, w in [(8.0, 1.0), (8.0, 4.0), (8.0, 100.0), (8.0, 0.999), (3.7, 0.01), (0.0, 0.0), (5.0, float("nan"))]:
        k, x = 0, np.float32(rw)
        while True:
            x = np.float32(float(x) / 2.0)
            k += 1
            if not float(x) / 2.0 > float(np.float32(w)):
                break
        assert host.L.st_depth_alone(rw, w) == k, (rw, w)


def test_non_finite_root_is_refused(host):
    center = np.array([[0, 0, 0, 1], [np.inf, 1, 1, 1]], np.float32)
    rc, _ = host.tree(center, np.ones(2, np.float32), None, 9)
    assert rc == HPMVS_ERR_ARG
