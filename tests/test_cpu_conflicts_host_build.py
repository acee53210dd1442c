"""The host build of a level's conflict graph that the C++ walk uses by default and as the fallback of HPMVS_DEVICE_GRAPH=1 (hpmvs_host.cpp:
clear_event_reads, build_conflict_graph, add_event_edges, reached through the hook hpmvs_host_conflict_graph) gives, with its
lists sorted, the bytes of the definition in tests/conflicts_ref.py -- so the graph the device call returns (held to the same
definition in tests/test_gpu_conflicts.py) can take its place in walk_level without moving a result."""
import ctypes as C
import os

import numpy as np
import pytest

import conflicts_ref as cr

LIB = os.path.join(cr.ROOT, "hpmvs_amd", "libhpmvs_host.so")
_lib = []


def host_lib():
    if not _lib:
        if not os.path.exists(LIB):   # (a fresh checkout: built as tests/test_cpu_filter.py's host_lib does)
            import subprocess
            subprocess.check_call(["make", "-C", os.path.join(cr.ROOT, "hpmvs_amd", "csrc")])
            subprocess.check_call(["make", "-C", os.path.join(cr.ROOT, "hpmvs_amd", "host")])
        _lib.append(C.CDLL(LIB))
    return _lib[0]


def host_build(ni, wr, fr, at, vb, n_levels, ev, max_w=1600, max_h=1200):
    L = host_lib()
    L.hpmvs_host_conflict_graph.argtypes = [C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    fo, ao = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    fa, aa = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    nf, na = C.c_uint32(0), C.c_uint32(0)
    for _ in range(2):
        rc = L.hpmvs_host_conflict_graph(n, M, V, n_levels, max_w, max_h, ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data,
                                         vb.ctypes.data, None if ev is None else ev.ctypes.data, fo.ctypes.data, fa.ctypes.data, fa.size,
                                         ao.ctypes.data, aa.ctypes.data, aa.size, C.byref(nf), C.byref(na))
        if rc != -2:
            break
        fa, aa = np.zeros(nf.value, np.uint32), np.zeros(na.value, np.uint32)
    assert rc == 0, rc
    return fo, fa, ao, aa


@pytest.mark.parametrize("case", [c for c in cr.RANDOM_CASES if c[1] <= 700], ids=lambda c: "n%d-V%d-L%d-M%d-ev%d" % c[1:6])
def test_host_build_equals_the_definition(case):
    ni, wr, fr, at, vb, ev, n_levels = cr.random_case(case)
    want = cr.definition(ni, wr, fr, at, vb, n_levels, ev)
    assert cr.graph_bytes(host_build(ni, wr, fr, at, vb, n_levels, ev)) == cr.graph_bytes(want)


@pytest.mark.parametrize("case", cr.known_answers(), ids=lambda c: c[0])
def test_host_build_on_the_known_answers(case):
    name, ni, wr, fr, at, vb, ev, n_levels, flow, anti = case
    assert cr.graph_bytes(host_build(ni, wr, fr, at, vb, n_levels, ev, 64, 64)) == cr.graph_bytes(cr.csr_of(flow) + cr.csr_of(anti)), name
