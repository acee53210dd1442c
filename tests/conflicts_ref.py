"""Test infrastructure for the conflict graph of an extend level (hpmvs_level_conflicts_batch, hpmvs_conflicts_from_footprints;
DESIGN.md §3.18), shared by the CPU and GPU tests:
  * definition(): the graph by brute-force set intersection in Python, straight from footprint arrays -- every node's read cells
    and written cells as sets of (view, level, x, y), and the four rules of include/hpmvs_amd.h over them;
  * HostConflicts: hpmvs_amd/csrc/conflicts.hpp's conflicts_sequential compiled by g++ (tests/conflicts_host.cpp);
  * random_footprints(): blocks at the image corners and beyond them, writes on every level, cells that collide, events;
  * known_answers(): cases written out by hand, each with the edges it must give."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "conflicts_host.cpp")
COORD_LIMIT = 1 << 24


def block_cells(view, ix0, iy0, n_levels, V, out):
    """The cells getFullDepth visits for the 3x3 level-0 pixel block from (ix0, iy0), every level."""
    if view < 0 or view >= V or ix0 < -2 or iy0 < -2 or ix0 >= COORD_LIMIT or iy0 >= COORD_LIMIT:
        return
    x1, y1, x0, y0 = ix0 + 2, iy0 + 2, max(ix0, 0), max(iy0, 0)
    for l in range(n_levels):
        for x in range(x0 >> (1 + l), (x1 >> (1 + l)) + 1):
            for y in range(y0 >> (1 + l), (y1 >> (1 + l)) + 1):
                out.add((view, l, x, y))


def _cell(e, n_levels, V):
    v, l, x, y = (int(a) for a in e)
    if v < 0 or v >= V or l < 0 or l >= n_levels or not (0 <= x < COORD_LIMIT) or not (0 <= y < COORD_LIMIT):
        return None
    return (v, l, x, y)


def cell_sets(n_images, wr, fr, at, vb, n_levels, is_event=None):
    """(reads, writes): per node the set of cells its gates read (empty for an event) and the set setDepths would write."""
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    R, W = [set() for _ in range(n)], [set() for _ in range(n)]
    for i in range(n):
        m = min(max(int(n_images[i]), 0), M)
        for k in range(m):
            c = _cell(wr[i, k], n_levels, V)
            if c is not None:
                W[i].add(c)
        if is_event is not None and is_event[i]:
            continue
        for k in range(m):
            c = _cell(fr[i, k], n_levels, V)
            if c is not None:
                R[i].add(c)
            block_cells(int(at[i, k, 0]), int(at[i, k, 1]), int(at[i, k, 2]), n_levels, V, R[i])
        for v in range(V):
            if vb[i, v, 0]:
                block_cells(v, int(vb[i, v, 1]), int(vb[i, v, 2]), n_levels, V, R[i])
    return R, W


def definition(n_images, wr, fr, at, vb, n_levels, is_event=None):
    """(flow_off, flow_adj, anti_off, anti_adj), uint32, lists ascending: the rules of include/hpmvs_amd.h over the cell sets.
    "j writes a cell i reads" is looked up through cell -> writers / readers tables: the same intersections, found without
    testing every pair of nodes."""
    n = wr.shape[0]
    ev = np.zeros(n, bool) if is_event is None else np.asarray(is_event).astype(bool)
    R, W = cell_sets(n_images, wr, fr, at, vb, n_levels, ev)
    writers, readers = {}, {}
    for i in range(n):
        for c in W[i]:
            writers.setdefault(c, []).append(i)
        for c in R[i]:
            readers.setdefault(c, []).append(i)
    flow, anti = [], []
    for i in range(n):
        f, a = set(), set()
        if ev[i]:
            for c in W[i]:
                f.update(j for j in writers[c] if j < i and not ev[j])
                a.update(j for j in readers.get(c, ()) if j < i)          # (readers are candidates: an event reads nothing)
        else:
            for c in R[i]:
                f.update(j for j in writers.get(c, ()) if j < i)
            for c in W[i]:
                a.update(j for j in readers.get(c, ()) if j < i)
                a.update(j for j in writers[c] if j < i and ev[j])
        flow.append(sorted(f)); anti.append(sorted(a))

    def csr(lists):
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in lists])
        return off, np.array([j for x in lists for j in x], np.uint32)
    return csr(flow) + csr(anti)


def graph_bytes(g):
    return tuple(np.ascontiguousarray(a, dtype=np.uint32).tobytes() for a in g)


class HostConflicts:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libconflicts_host.so")
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        self.L = C.CDLL(so)
        self.L.cf_conflicts.argtypes = [C.c_int] * 4 + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def graph(self, n_images, wr, fr, at, vb, n_levels, is_event=None):
        n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
        ni = np.ascontiguousarray(n_images, np.int32)
        ev = None if is_event is None else np.ascontiguousarray(is_event, np.uint8)
        fo, ao = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        nf, na = C.c_uint32(0), C.c_uint32(0)
        fa, aa = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        for _ in range(2):   # the capacity contract: sized by the first call
            rc = self.L.cf_conflicts(n, M, V, n_levels, ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data, vb.ctypes.data,
                                     None if ev is None else ev.ctypes.data, fo.ctypes.data, fa.ctypes.data, fa.size, ao.ctypes.data,
                                     aa.ctypes.data, aa.size, C.byref(nf), C.byref(na))
            if rc != -2:
                break
            fa, aa = np.zeros(nf.value, np.uint32), np.zeros(na.value, np.uint32)
        assert rc == 0, rc
        return fo, fa, ao, aa


def empty_footprints(n, M, V):
    return (np.zeros(n, np.int32), np.full((n, M, 4), -1, np.int32), np.full((n, M, 4), -1, np.int32), np.full((n, M, 3), -1, np.int32),
            np.zeros((n, V, 3), np.int32))


def random_footprints(seed, n, V, max_w, max_h, n_levels, M, event_every=0, window=24):
    """The scheme of the host layer's selftest footprints: everything happens in windows at the four image corners, where blocks
    reach outside the image, so that nodes really meet; writes and pixelFreeTests cells on random levels next to the node's
    pixel.  event_every = 3: every third node is an event.  Some rows are shorter than M, some nodes have no image.
    Returns (n_images, wr, fr, at, vb, is_event or None)."""
    rng = np.random.default_rng(seed)
    ni, wr, fr, at, vb = empty_footprints(n, M, V)
    wx, wy = min(max_w // 4, window), min(max_h // 4, window)
    for i in range(n):
        m = int(rng.integers(0, M + 1)) if rng.integers(0, 10) == 0 else int(rng.integers(1, M + 1))
        ni[i] = m
        corner = int(rng.integers(0, 4))
        bx = max_w - wx - 1 if corner & 1 else -2
        by = max_h - wy - 1 if corner & 2 else -2
        for k in range(m):
            view = int(rng.integers(0, V)); px = bx + int(rng.integers(0, wx + 3)); py = by + int(rng.integers(0, wy + 3))
            if rng.integers(0, 8):
                at[i, k] = (view, px - 1, py - 1)
            l = int(rng.integers(0, n_levels))
            if rng.integers(0, 6):
                wr[i, k] = (view, l, (max(px, 0) >> (1 + l)) + int(rng.integers(0, 2)), (max(py, 0) >> (1 + l)) + int(rng.integers(0, 2)))
            lf = int(rng.integers(0, n_levels))
            if rng.integers(0, 6):
                fr[i, k] = (view, lf, (max(px, 0) >> (1 + lf)) + int(rng.integers(0, 2)), (max(py, 0) >> (1 + lf)) + int(rng.integers(0, 2)))
        for v in range(V):
            if rng.integers(0, 3) == 0:
                vb[i, v] = (1, bx + int(rng.integers(0, wx + 3)) - 1, by + int(rng.integers(0, wy + 3)) - 1)
    ev = None
    if event_every:
        ev = (np.arange(n) % event_every == event_every - 1).astype(np.uint8)
    return ni, wr, fr, at, vb, ev


# The random cases of the host-restatement test and of the GPU test: (seed, n, V, n_levels, M, event_every, window).  Every n of
# {1, 2, 65, 700, 2500}, every V of {1, 3, 50}, n_levels 1 .. 8, every M of {1, 7, 70} (70: more images than a wavefront has
# lanes); the large ones in wide windows, so that the graph stays a graph and not all pairs.
RANDOM_CASES = [
    (1, 1, 1, 1, 1, 0, 24), (2, 2, 3, 2, 7, 0, 24), (3, 2, 1, 3, 1, 3, 24), (4, 65, 3, 4, 7, 3, 24), (5, 65, 50, 5, 70, 0, 24),
    (6, 65, 1, 6, 70, 3, 24), (7, 700, 3, 7, 7, 3, 120), (8, 700, 50, 8, 1, 0, 60), (9, 2500, 3, 6, 7, 3, 400), (10, 65, 3, 8, 7, 3, 24),
]


def random_case(case):
    seed, n, V, n_levels, M, event_every, window = case
    return random_footprints(seed, n, V, 1600, 1200, n_levels, M, event_every, window) + (n_levels,)


def known_answers():
    """Hand-written cases: (name, n_images, wr, fr, at, vb, is_event, n_levels, flow lists, anti lists)."""
    out = []

    def case(name, n, M, V, n_levels, fill, flow, anti, events=None):
        ni, wr, fr, at, vb = empty_footprints(n, M, V)
        fill(ni, wr, fr, at, vb)
        ev = None if events is None else np.array(events, np.uint8)
        out.append((name, ni, wr, fr, at, vb, ev, n_levels, flow, anti))

    # node 1 reads the block from (5, 5): pixels 5 .. 7, level-0 cells 2 .. 3 (straddles), level-2 cell 0 only.  Node 0 writes
    # level-0 cell (3, 3): inside.  Node 2 writes level-0 cell (4, 3): outside; node 3 level-2 cell (0, 0): inside; node 4 level-2
    # cell (1, 0): outside (on level 2 the block does not straddle).  Later writers land in anti of their own lists.
    def straddle(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[0, 0] = (0, 0, 3, 3); at[1, 0] = (0, 5, 5); wr[2, 0] = (0, 0, 4, 3); wr[3, 0] = (0, 2, 0, 0); wr[4, 0] = (0, 2, 1, 0)
    case("a block straddling a cell boundary on level 0 but not on level 2", 5, 1, 1, 3, straddle,
         [[], [0], [], [], []], [[], [], [], [1], []])

    # block at (-2, -2): x1 = 0, cell 0 only, every level; block at (-3, 5): x1 < 0, none
    def corner(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[0, 0] = (1, 0, 0, 0); wr[1, 0] = (1, 1, 0, 0); wr[2, 0] = (1, 0, 1, 0); wr[3, 0] = (1, 0, 0, 2)
        vb[4, 1] = (1, -2, -2); vb[5, 1] = (1, -3, 5)
    case("a block at (-2, -2) (cell 0 only) and at (-3, 5) (none)", 6, 1, 2, 2, corner,
         [[], [], [], [], [0, 1], []], [[]] * 6)

    # a write on level n_levels - 1 is met by a block; one on level n_levels is on no level the gates read
    def top(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[0, 0] = (0, 3, 1, 1); wr[1, 0] = (0, 4, 0, 0); at[2, 0] = (0, 30, 30); fr[2, 0] = (0, 4, 0, 0)
    case("a write on level n_levels - 1", 3, 1, 1, 4, top, [[], [], [0]], [[]] * 3)

    # view == V: ignored as a write, as a pixelFreeTests read and as a block
    def view_v(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[0, 0] = (2, 0, 5, 5); fr[1, 0] = (2, 0, 5, 5); at[1, 0] = (2, 10, 10); wr[2, 0] = (1, 0, 5, 5); fr[3, 0] = (1, 0, 5, 5)
    case("a write with view == V (ignored)", 4, 1, 2, 1, view_v, [[], [], [], [2]], [[]] * 4)

    # eight images of node 0 write the cell all eight images of node 1 read (free cell and block): ONE edge
    def eight(ni, wr, fr, at, vb):
        ni[:] = 8
        wr[0, :] = (0, 1, 3, 4); fr[1, :] = (0, 1, 3, 4); at[1, :] = (0, 12, 16)
    case("two nodes whose eight images all hit one cell (one edge, not eight)", 2, 8, 1, 2, eight, [[], [0]], [[], []])

    # event 0, candidate 1, event 2 all write cell c; candidate 1 also reads it.  flow[1] = {0} (an event's write it reads),
    # anti[1] = {0} (an earlier event writes what it writes), flow[2] = {1} (write-write), anti[2] = {1} (1 reads what 2 writes)
    def ev_around(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[:, 0] = (0, 0, 7, 7); fr[1, 0] = (0, 0, 7, 7); fr[0, 0] = (0, 0, 7, 7); at[2, 0] = (0, 14, 14)   # (events' reads: ignored)
    case("an event before and after a candidate on the same cell", 3, 1, 1, 1, ev_around, [[], [0], [1]], [[], [0], [1]], [1, 0, 1])

    def two_events(ni, wr, fr, at, vb):
        ni[:] = 1
        wr[:, 0] = (0, 0, 2, 2); fr[:, 0] = (0, 0, 2, 2)
    case("two events on one cell (no edge)", 2, 1, 1, 1, two_events, [[], []], [[], []], [1, 1])

    # the entries past n_images do not count; a node without images is valid
    def rows(ni, wr, fr, at, vb):
        ni[:] = (2, 0, 1)
        wr[0, :] = (0, 0, 1, 1); wr[1, :] = (0, 0, 1, 1); fr[2, 0] = (0, 0, 9, 9); fr[2, 1] = (0, 0, 1, 1); fr[2, 2] = (0, 0, 1, 1)
    case("entries past n_images and a node with no image", 3, 3, 1, 1, rows, [[], [], []], [[], [], []])
    return out


def csr_of(lists):
    off = np.zeros(len(lists) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([j for x in lists for j in x], np.uint32)
