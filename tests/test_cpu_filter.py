"""Host side of the filter path (reference src/hpmvs/CellProcessor.cpp:43-82) that needs no device: the float32
restatement of filter (tests/filter_ref.py) on cells computed by hand, the C entry's refusal to run without a GPU, the Python
level calls' refusal of malformed offsets, and the conflict graph of PatchOptimizer::filterExtendLevel -- candidates plus
subtraction events -- against its definition by brute-force set intersection (`hpmvs_host_selftest_event_graph`)."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _cell(centres, normals):
    c = np.array([list(p) + [1.0] for p in centres], f32)
    n = np.array([list(p) + [0.0] for p in normals], f32)
    return c, n


def test_two_patches_keep_the_one_the_other_lies_below():
    # n0 . (c1 - c0) = 1, n1 . (c0 - c1) = -1: the second patch has the smaller (signed) distance
    c, n = _cell([(0, 0, 0), (0, 0, 1)], [(0, 0, 1), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d.tolist() == [1.0, -1.0] and k == 1


def test_three_patches_signed_mean_and_unnormalised_normals():
    # normals of length 2 and 4 are normalised first; distances are summed with their sign and divided by k - 1 = 2
    c, n = _cell([(0, 0, 0), (0, 0, 2), (0, 0, -4)], [(0, 0, 2), (0, 0, 4), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d.tolist() == [(2.0 - 4.0) / 2, (-2.0 - 6.0) / 2, (4.0 + 6.0) / 2] and k == 1


def test_exact_ties_keep_the_lowest_index():
    # two patches mirrored through the plane of a third: rows 0 and 1 tie exactly
    c, n = _cell([(1, 0, 0), (-1, 0, 0), (0, 0, 1)], [(0, 0, 1), (0, 0, 1), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d[0] == d[1] == f32(0.5) and d[2] == f32(-1.0) and k == 2
    c, n = _cell([(0, 0, 0), (0, 0, 0), (0, 0, 0)], [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d.tolist() == [0.0, 0.0, 0.0] and k == 0


def test_zero_normals_nan_and_inf_never_win_a_cell_without_winner():
    # a zero normal stays zero: its distance is 0
    c, n = _cell([(0, 0, 0), (0, 0, 1), (0, 0, 2)], [(0, 0, 0), (0, 0, 1), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d.tolist() == [0.0, 0.0, -1.5] and k == 2
    c, n = _cell([(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert d.tolist() == [0.0, -1.0] and k == 1
    # a NaN centre poisons every row's sum: no distance below FLT_MAX, no winner
    c, n = _cell([(0, 0, np.nan), (0, 0, 1), (0, 0, 2)], [(0, 0, 1)] * 3)
    d, k = fr.filter_cell(c, n)
    assert np.isnan(d).all() and k is None
    # +inf distances never win ...
    c, n = _cell([(0, 0, np.inf), (0, 0, 0)], [(0, 0, -1), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert np.isposinf(d).all() and k is None
    # ... -inf does
    c, n = _cell([(0, 0, 0), (0, 0, 1), (0, 0, np.inf)], [(0, 0, 1), (0, 0, 1), (0, 0, 1)])
    d, k = fr.filter_cell(c, n)
    assert np.isposinf(d[:2]).all() and np.isneginf(d[2]) and k == 2
    # exactly FLT_MAX is not below FLT_MAX
    c, n = _cell([(0, 0, 0), (0, 0, float(np.finfo(np.float32).max))], [(0, 0, 1), (1, 0, 0)])
    d, k = fr.filter_cell(c, n)
    assert d[0] == np.finfo(np.float32).max and k == 1


def test_filter_cells_codes():
    c, n = _cell([(0, 0, 0), (0, 0, 1), (5, 5, 5), (0, 0, np.nan), (0, 0, 1)], [(0, 0, 1)] * 5)
    d, keep = fr.filter_cells(c, n, [0, 2, 2, 3, 5])
    assert keep.tolist() == [1, -1, 2, -2]
    assert d[2] == 0.0


def test_filter_batch_has_no_cpu_fallback():
    from hpmvs_amd import api
    if api.device_count() > 0:
        return  # on a GPU box tests/test_gpu_filter_level.py covers the call
    b = api.Batch(np.zeros((2, 4)), np.zeros((2, 4)), np.zeros(2), np.ones(2), np.zeros((2, 1)))
    cs = np.array([0, 2], np.int32)
    d, k = np.zeros(2, np.float32), np.zeros(1, np.int32)
    rc = api.lib().hpmvs_filter_batch(None, C.byref(b.c_struct()), cs.ctypes.data, 1, d.ctypes.data, k.ctypes.data, 0, None)
    assert rc == -4  # HPMVS_ERR_NODEVICE


@pytest.mark.parametrize("cs", [[1, 3], [0, 2, 1, 3], [0, 2], [0, 4]])
def test_level_calls_refuse_malformed_offsets(cs):
    from hpmvs_amd import api, frontier
    b = api.Batch(np.zeros((3, 4)), np.zeros((3, 4)), np.zeros(3), np.ones(3), np.zeros((3, 1)))
    with pytest.raises(ValueError):
        frontier.filter_level(None, b, cs)


@pytest.fixture(scope="module")
def host_lib():
    import __graft_entry__  # noqa: F401  (puts the repo root on sys.path)
    path = os.path.join(ROOT, "hpmvs_amd", "libhpmvs_host.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "hpmvs_amd", "csrc")])
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "hpmvs_amd", "host")])
    L = C.CDLL(path)
    L.hpmvs_host_selftest_event_graph.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


@pytest.mark.parametrize("seed,n,views,w,h,levels,m,every", [
    (1, 300, 3, 640, 480, 6, 3, 3),
    (2, 1200, 12, 1920, 1080, 6, 8, 2),
    (3, 2500, 50, 3840, 2160, 6, 12, 4),   # above the OpenMP threshold of build_conflict_graph
    (4, 400, 2, 64, 48, 6, 4, 5),
    (5, 300, 3, 640, 480, 6, 3, 1),        # every node an event: no edge at all
])
def test_event_graph_equals_the_definition(host_lib, seed, n, views, w, h, levels, m, every):
    edges, events = C.c_int(-1), C.c_int(-1)
    assert host_lib.hpmvs_host_selftest_event_graph(seed, n, views, w, h, levels, m, every, C.byref(edges), C.byref(events)) == 0
    print("event graph:", n, "nodes,", events.value, "events,", edges.value, "edges")
    if every == 1:
        assert events.value == n and edges.value == 0
    else:
        assert 0 < events.value < n and edges.value >= 5 * n   # the footprints do meet


def test_event_graph_selftest_refuses_bad_arguments(host_lib):
    assert host_lib.hpmvs_host_selftest_event_graph(1, 10, 3, 640, 480, 6, 3, 0, None, None) == -1
    assert host_lib.hpmvs_host_selftest_event_graph(1, 0, 3, 640, 480, 6, 3, 2, None, None) == -1
