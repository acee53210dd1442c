"""The conflict graph of an extend level, host side.  Three statements of one definition are held against each
other: the edges written out by hand for small cases, the definition by brute-force set intersection in Python
(tests/conflicts_ref.py), and the g++ build of hpmvs_amd/csrc/conflicts.hpp's conflicts_sequential (tests/conflicts_host.cpp) --
the restatement the device kernels share their cell enumeration with, which must equal the Python definition byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import conflicts_ref as cr


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cr.HostConflicts(tmp_path_factory.mktemp("conflicts_host"))


@pytest.mark.parametrize("case", cr.known_answers(), ids=lambda c: c[0])
def test_known_answers(host, case):
    name, ni, wr, fr, at, vb, ev, n_levels, flow, anti = case
    want = cr.graph_bytes(cr.csr_of(flow) + cr.csr_of(anti))
    assert cr.graph_bytes(cr.definition(ni, wr, fr, at, vb, n_levels, ev)) == want, name
    assert cr.graph_bytes(host.graph(ni, wr, fr, at, vb, n_levels, ev)) == want, name


@pytest.mark.parametrize("case", cr.RANDOM_CASES, ids=lambda c: "n%d-V%d-L%d-M%d-ev%d" % c[1:6])
def test_host_restatement_equals_the_definition(host, case):
    ni, wr, fr, at, vb, ev, n_levels = cr.random_case(case)
    want = cr.definition(ni, wr, fr, at, vb, n_levels, ev)
    got = host.graph(ni, wr, fr, at, vb, n_levels, ev)
    assert cr.graph_bytes(got) == cr.graph_bytes(want)
    n = wr.shape[0]
    if n >= 65:   # the case is a graph: nodes meet, and not every pair does
        edges = len(want[1]) + len(want[3])
        assert 0 < edges < n * (n - 1) // 2, edges
    for off, adj in ((got[0], got[1]), (got[2], got[3])):
        for i in range(n):
            row = adj[off[i]:off[i + 1]]
            assert np.all(row[1:] > row[:-1]) and np.all(row < i)   # ascending, no duplicate, earlier nodes only


def test_events_have_no_reads_and_no_edges_among_themselves(host):
    ni, wr, fr, at, vb, ev, n_levels = cr.random_case((11, 200, 3, 4, 7, 2, 24))
    fo, fa, ao, aa = host.graph(ni, wr, fr, at, vb, n_levels, ev)
    for i in np.nonzero(ev)[0]:
        assert not ev[fa[fo[i]:fo[i + 1]]].any() and not ev[aa[ao[i]:ao[i + 1]]].any()
    # with the events' read entries cleared the graph is the same: they never counted
    fr2, at2, vb2 = fr.copy(), at.copy(), vb.copy()
    fr2[ev != 0] = -1; at2[ev != 0] = -1; vb2[ev != 0] = 0
    assert cr.graph_bytes(host.graph(ni, wr, fr2, at2, vb2, n_levels, ev)) == cr.graph_bytes((fo, fa, ao, aa))


def test_every_node_on_one_cell_is_refused_before_anything_is_walked_or_written(host):
    """3072 nodes, 8 images each, all on cell (1, 1) of one map: each node's 8 free cells and 8 blocks hold all 24 576 write
    records, 3072 x 16 x 24 576 = 1.2e9 matches > 2^30.  The refusal comes from two bounds per key range (about 5e4 ranges), not
    from a walk over the 1.2e9 pairs: the call returns at once."""
    import ctypes as C
    n, M = 3072, 8
    ni, wr, fr, at, vb = cr.empty_footprints(n, M, 1)
    ni[:] = M; wr[:] = (0, 0, 1, 1); fr[:] = (0, 0, 1, 1); at[:] = (0, 2, 2)
    poison = 0xDEADBEEF
    fo, ao = np.full(n + 1, poison, np.uint32), np.full(n + 1, poison, np.uint32)
    fa, aa = np.full(64, poison, np.uint32), np.full(64, poison, np.uint32)
    nf, na = C.c_uint32(poison), C.c_uint32(poison)
    rc = host.L.cf_conflicts(n, M, 1, 1, ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data, vb.ctypes.data, None, fo.ctypes.data,
                             fa.ctypes.data, fa.size, ao.ctypes.data, aa.ctypes.data, aa.size, C.byref(nf), C.byref(na))
    assert rc == -3
    assert (nf.value, na.value) == (poison, poison) and all((a == poison).all() for a in (fo, ao, fa, aa))


def test_the_stand_alone_selftest_runs_clean_under_the_sanitizers(tmp_path):
    """tests/native/conflicts_selftest.cpp: conflicts_sequential against an in-program definition of its own, a program of its
    own built with AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "conflicts_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cr.ROOT, "tests", "native", "conflicts_selftest.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
