"""The text of the patch cloud's PLY file, on the host: hpmvs_amd/csrc/ply_text.hpp compiled with g++ (tests/ply_text_host.cpp)
against the pin.

The pin is this machine's glibc and libstdc++: snprintf("%.6g", (double)f), which is what libstdc++'s operator<<(float) calls
with default flags, and Python's '%.6g' % float(np.float32(v)), which is exact too; the unchanged host mo3d::writeExtPly writes
with the same iostream calls (tests/test_gpu_cpp_to_ext_ply.py compares files with it).  The reference's own translation units
cannot be compiled where the fixtures are made (no Eigen), so no file of the reference's is a fixture here.

tools/ply_text_sweep.cpp compares ALL 2^32 bit patterns (profiles/ply_text_sweep.json: 0 mismatches); here a strided sample,
the contract's values, every decade's boundaries and constructed exact ties."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

import ply_ref as ref


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ref.HostPlyText(tmp_path_factory.mktemp("ply_text_host"))


def bits_of(values):
    return np.array(values, dtype=np.float32).view(np.uint32)


def test_every_4099th_pattern_equals_snprintf(host):
    count = (2 ** 32 + 4098) // 4099   # both signs, denormals, infinities, NaNs
    bad, first = host.check_snprintf(0, 4099, count)
    assert count > 1_040_000 and bad == 0, hex(first)


def test_contract_values(host):
    got = host.format(bits_of([v for v, _ in ref.CONTRACT]))
    assert got == [t for _, t in ref.CONTRACT]
    assert got == [ref.fmt(np.float32(v)) for v, _ in ref.CONTRACT]
    assert host.format([b for b, _ in ref.NANS]) == [t for _, t in ref.NANS]
    sp = ref.special_bits()
    assert host.check_list(sp)[0] == 0 and host.format(sp) == [ref.fmt(v) for v in sp.view(np.float32)]
    assert max(len(t) for t in host.format(sp)) == 12   # the longest field


def test_decade_boundaries(host):
    """for each decimal exponent -45 .. 38 the floats nearest below, at and above 10^X and 9.999995 * 10^X: where the notation
    changes, where a carry out of 999999 moves the exponent"""
    vals = []
    for X in range(-45, 39):
        for mant in ("1", "9.999995"):
            d = float(Decimal(mant).scaleb(X))
            if d > 3.4028234663852886e38:
                continue
            v = np.float32(d)
            vals += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    vals = np.array(vals, np.float32)
    vals = vals[np.isfinite(vals)]
    both = np.concatenate([vals, -vals]).view(np.uint32)
    assert len(both) > 900
    bad, first = host.check_list(both)
    assert bad == 0, hex(first)
    assert host.format(both) == [ref.fmt(v) for v in both.view(np.float32)]


def test_exact_ties_round_to_even(host):
    """10 000 floats whose exact value has seven significant digits, the last a 5: the integers 10 k + 5 (k = 100000 .. 999999,
    all below 2^24) and their products with powers of two, 2^-4 .. 2^4, that still are such ties.  For k in this range only
    2^-1 (5 k + 2.5 with k < 200000: the fractional path, a sticky bit of exactly zero behind a nonzero chunk) and 2^1
    (20 k + 10 with 2 k + 1 a multiple of 5, k >= 500000: a value above 2^24) give any: a tie at the seventh digit needs
    (10 k + 5) 2^j = (2 q + 1) 5 * 10^(j) with six digits in q.  Every power that gives ties takes part with up to 1000 of
    them, the integers fill the rest; both directions must occur, among the integers and among the products."""
    POWERS = (-4, -3, -2, -1, 1, 2, 3, 4)
    found = {j: [] for j in (0,) + POWERS}   # j -> (value, text wanted, rounds up)
    for j in found:
        for k in range(100000, 1000000, 7 if j else 61):
            v = (10 * k + 5) * 2.0 ** j
            if float(np.float32(v)) != v:
                continue
            sign, digits, exp = Decimal(v).normalize().as_tuple()
            if len(digits) != 7 or digits[-1] != 5:
                continue
            q = int("".join(map(str, digits[:6])))
            q += q & 1   # half-even
            found[j].append((v, "%.6g" % float(Decimal(q).scaleb(exp + 1)), bool(digits[5] & 1)))
    assert len(found[-1]) >= 1000 and len(found[1]) >= 1000, {j: len(t) for j, t in found.items()}
    assert any(v != int(v) for v, _, _ in found[-1])   # fractions are among them
    products = [t for j in POWERS for t in found[j][:1000]]
    ties = products + found[0][:10000 - len(products)]
    assert len(ties) == 10000 and len(products) >= 2000
    for group in (products, found[0][:10000 - len(products)]):
        ups = sum(up for _, _, up in group)
        assert ups > len(group) // 4 and len(group) - ups > len(group) // 4
    b = bits_of([v for v, _, _ in ties])
    assert host.check_list(b)[0] == 0
    got = host.format(b)
    assert got == [w for _, w, _ in ties] and got == [ref.fmt(v) for v in b.view(np.float32)]


def test_colour_rule(host):
    vals = np.array([0.0, -0.0, 0.99, 1.0, 1.99, 2.0, 17.99, 127.5, 128.0, 254.999, 255.0, 255.99, 256.0, 1e9, -0.5, -3.0, np.inf, -np.inf, np.nan,
                     1e-45, 3.4e38], np.float32)
    assert host.colour_bytes(vals).tolist() == [ref.colour(v) for v in vals]
    inside = np.linspace(0, 255.996, 4001).astype(np.float32)   # where (unsigned char) of the float is defined: truncation
    assert (host.colour_bytes(inside) == inside.astype(np.uint8)).all()
    nan_neg = np.array([0xFFC00000], np.uint32).view(np.float32)
    assert host.colour_bytes(nan_neg).tolist() == [0]


@pytest.mark.parametrize("flags", range(16))
def test_file_of_the_host_restatement(host, flags):
    rows = ref.Rows(65, max_images=64, seed=7)
    assert host.file(rows, None, flags) == ref.build(rows, None, flags)
    order = [3, 3, 64, 0, 1, 1, 17]
    assert host.file(rows, order, flags) == ref.build(rows, order, flags)
    empty = ref.Rows(0, max_images=4, seed=1)
    assert host.file(empty, None, flags) == ref.header(0, flags)


def test_argument_checks_come_before_the_device():
    """each is refused as HPMVS_ERR_ARG (-2) whether or not a device is visible: HPMVS_ERR_NODEVICE (-4) would come later"""
    from hpmvs_amd import api
    L = api.lib()
    n, b = C.c_size_t(0), api.PatchBatch()
    order = np.zeros(4, np.int32)
    out = np.zeros(64, np.uint8)
    call = lambda bp, order, n_rows, flags, outp, cap, np_: L.hpmvs_ply_ext_batch(0, bp, order, n_rows, flags, outp, cap, np_, 0, None)
    cases = {
        "null b": (None, None, 0, 14, None, 0, C.byref(n)),
        "null n": (C.byref(b), None, 0, 14, None, 0, None),
        "negative n_rows": (C.byref(b), order.ctypes.data, -1, 14, None, 0, C.byref(n)),
        "unknown flag bits": (C.byref(b), None, 0, 16, None, 0, C.byref(n)),
        "cap without out": (C.byref(b), None, 0, 14, None, 64, C.byref(n)),
    }
    for name, args in cases.items():
        assert call(*args) == -2, name
        assert "ply_ext_batch" in L.hpmvs_last_error().decode(), name
    b.n = -1
    assert call(C.byref(b), None, 0, 14, out.ctypes.data, 64, C.byref(n)) == -2
    b.n = 3   # rows without arrays
    assert call(C.byref(b), None, 0, 14, out.ctypes.data, 64, C.byref(n)) == -2
    ms = (C.c_float * 6)()
    assert L.hpmvs_ply_ext_timed(0, None, None, 0, 14, None, 0, C.byref(n), ms) == -2
    assert L.hpmvs_ply_ext_timed(0, C.byref(b), None, 0, 14, None, 0, C.byref(n), None) == -2


def test_forest_leaf_order_is_the_whole_trees_order():
    from hpmvs_amd import frontier
    rng = np.random.default_rng(11)
    tree = frontier.Octree([0.0, 0.0, 0.0], 8.0)
    row = 0
    for p in rng.uniform(-3.9, 3.9, (400, 3)).astype(np.float32):
        width = np.float32(8.0 / 2 ** int(rng.integers(2, 6)))
        data = list(range(row, row + int(rng.integers(1, 4))))   # a leaf's patches, in data order
        if tree.add_conditional(p, width, data) is not None:
            row += len(data)
    keys, rows, _, _ = tree.leaf_table()
    want = [r for data in rows for r in data]
    assert len(keys) > 100 and len(want) == row
    # a partition as getSubTrees leaves it: subtrees cut at different depths, in no particular order, and leaves in none of them
    depth1 = [k for k in range(8, 16) if k in tree.branches]
    depth2 = [k for k in sorted(tree.branches) if frontier.key_depth(k) == 2 and (k >> 3) == depth1[0]]
    assert len(depth1) >= 4 and len(depth2) >= 2
    roots = [depth1[3], depth2[1], depth1[1], depth2[0]]
    trees = [tree.subtree(k) for k in roots]
    below = lambda k, root: (k >> (3 * (frontier.key_depth(k) - frontier.key_depth(root)))) == root if frontier.key_depth(k) > frontier.key_depth(root) else False
    orphans = [(int(k), tree.leaves[int(k)]) for k in keys if not any(below(int(k), r) for r in roots)]
    assert orphans and sum(len(t.leaves) for t in trees) + len(orphans) == len(keys)
    order = frontier.forest_leaf_order(trees, roots, orphans)
    assert order.dtype == np.int32 and order.tolist() == want
    assert frontier.forest_leaf_order([tree], [frontier.Octree.ROOT]).tolist() == want   # the root alone
    assert frontier.forest_leaf_order(trees, roots).tolist() != want                    # (the orphans matter)
