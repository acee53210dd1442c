"""The per-round exchange on the device, at the shapes a real round has: hpmvs_pack_records / hpmvs_unpack_records /
hpmvs_pack_record_tails / hpmvs_unpack_record_tails through the C ABI with device pointers, compared BYTE FOR BYTE with
tests/record_ref.py (a reading of include/hpmvs_amd.h that shares nothing with the kernels).  No tolerances.

Every output buffer is filled with 0x5A (and every destination column with a sentinel) before each call, so that pad bytes,
slots past n_tails, slots past `cap` and rows a call must not touch are checked as well.  Buffers are allocated with room
beyond what a call may write, and destinations of the offset tests with guard rows on both sides, and both are compared in
full.  The cases' preconditions (tails beyond the scan's first chunk, empty runs, full blocks ...) are asserted in
tests/test_cpu_record_ref.py.
"""
import ctypes as C

import numpy as np
import pytest

import record_ref as rr

pytestmark = pytest.mark.gpu

HPMVS_ERR_ARG = -2
FILL = 0x5A


@pytest.fixture(scope="module")
def L():
    from hpmvs_amd import api
    lib = api.lib()
    lib.hpmvs_pack_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hpmvs_unpack_records.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.hpmvs_pack_record_tails.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    lib.hpmvs_unpack_record_tails.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    return lib


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _filled(rows, width):
    import torch
    return torch.full((rows, width), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy()


def _as_tails(t):
    return np.frombuffer(_host(t).tobytes(), rr.TAIL)


def _as_bytes(a, width):
    return np.frombuffer(a.tobytes(), np.uint8).reshape(-1, width).copy()


def _same(got, want):
    """True when the rows of a uint8 buffer are the bytes of the reference's structured array; else fails with the first
    (row, byte) positions that differ instead of a dump of both."""
    want = _as_bytes(want, got.shape[1])
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("first differing (row, byte)", bad[:8].tolist())
    return True


def _batch(n, m, cols, lo=0):
    """hpmvs_patch_batch over rows lo.. of device columns; a column that is None (or missing) is handed over as NULL."""
    from hpmvs_amd import api
    b = api.PatchBatch()
    b.n, b.max_images = n, m
    b.cols = cols          # (the batch holds raw pointers: keep their tensors alive as long as it)
    for k, v in cols.items():
        if v is not None:
            setattr(b, k, v[lo:].data_ptr())
    return b


def _case_dev(c):
    """Every row of the case's columns on the device (the over-allocation past c.n too); absent optionals are None."""
    return {k: (None if k in c.absent else _dev(v)) for k, v in c.arrays.items()}


def _pack_tails(L, b, buf, cap, stream=None):
    nt = C.c_int32(-1)
    rc = L.hpmvs_pack_record_tails(C.byref(b), None if buf is None else buf.data_ptr(), cap, C.byref(nt), stream)
    return rc, nt.value


class Dst:
    """A sentinel-filled destination batch of n rows on the device with guard rows before and after it, and the same
    arrays on the host for the reference to unpack into."""

    def __init__(self, n, m, absent=(), front=0, back=3):
        self.n, self.m, self.front, self.absent = n, m, front, tuple(absent)
        self.host = rr.sentinel_batch(front + n + back, m)
        self.dev = {k: _dev(v) for k, v in self.host.items()}

    def batch(self):
        return _batch(self.n, self.m, {k: v for k, v in self.dev.items() if k not in self.absent}, self.front)

    def ref(self):
        return {k: (None if k in self.absent else v[self.front:self.front + self.n]) for k, v in self.host.items()}

    def got(self, key):
        return _host(self.dev[key])[self.front:self.front + self.n]

    def assert_equals_reference(self):
        for k, want in self.host.items():
            got = _host(self.dev[k])
            assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5].tolist())


SCAN_KEYS = [(n, p) for n in rr.SCAN_SIZES for p in rr.SCAN_PATTERNS]


@pytest.mark.parametrize("n,pattern", SCAN_KEYS, ids=[f"{p}-{n}" for n, p in SCAN_KEYS])
def test_tail_list_across_scan_chunks_and_block_edges(L, n, pattern):
    """hpmvs_pack_record_tails at max_images = 70: 1 .. 513 blocks of 64 patches, i.e. up to three chunks of the scan with
    its carry between them; the arrays go on past b.n with long lists that must not be counted."""
    import torch
    c = rr.scan_case(n, pattern)
    want = c.ref_tails()
    T = len(want)
    buf = _filled(T + 70, rr.TAIL.itemsize)
    cap = T if pattern == "c" else T + 70     # (pattern c: n_tails == n == cap)
    assert pattern != "c" or T == n
    rc, nt = _pack_tails(L, _batch(n, c.max_images, _case_dev(c)), buf, cap)
    torch.cuda.synchronize()
    assert rc == 0, L.hpmvs_last_error()
    assert nt == T
    got = _host(buf)
    patch = _as_tails(buf)["patch"][:T].astype(np.int64)
    assert np.all(np.diff(patch) > 0)
    assert np.array_equal(patch, want["patch"])
    assert _same(got[:T], want)
    assert np.all(got[T:] == FILL)


def test_tail_segment_capacity(L):
    """cap == n_tails fits; one short is refused with the true number and nothing past the cap-th tail written; no segment
    at all is fine exactly when there is no long list; rows of up to 64 ids never have tails."""
    import torch
    c = rr.case(rr.CAPACITY_KEY)
    want = c.ref_tails()
    T = len(want)
    assert T > 20
    cols = _case_dev(c)
    b = _batch(c.n, c.max_images, cols)
    # cap == n_tails exactly
    buf = _filled(T + 8, 392)
    assert _pack_tails(L, b, buf, T) == (0, T), L.hpmvs_last_error()
    torch.cuda.synchronize()
    assert _same(_host(buf)[:T], want) and np.all(_host(buf)[T:] == FILL)
    # one short: refused, the true number reported, nothing written past the cap-th tail
    buf = _filled(T + 8, 392)
    assert _pack_tails(L, b, buf, T - 1) == (HPMVS_ERR_ARG, T)
    torch.cuda.synchronize()
    assert np.all(_host(buf)[T - 1:] == FILL)
    # no segment at all: refused here ...
    assert _pack_tails(L, b, None, 0) == (HPMVS_ERR_ARG, T)
    # ... and fine for a batch without a long list (whose arrays go on past b.n with long lists)
    z = rr.case(rr.NO_LONG_KEY)
    assert len(z.ref_tails()) == 0
    assert _pack_tails(L, _batch(z.n, z.max_images, _case_dev(z)), None, 0) == (0, 0), L.hpmvs_last_error()
    # rows of up to 64 ids have no tails, whatever n_images says
    for m in (64, 5):
        w = rr.width_case(m)
        assert np.any(w.col("n_images") > 64)
        buf = _filled(8, 392)
        assert _pack_tails(L, _batch(w.n, m, _case_dev(w)), buf, 8) == (0, 0), L.hpmvs_last_error()
        torch.cuda.synchronize()
        assert np.all(_host(buf) == FILL)


WIDTH_KEYS = [(m, ()) for m in rr.WIDTHS] + [(100, a) for a in rr.ABSENT_COMBOS]


@pytest.mark.parametrize("m,absent", WIDTH_KEYS, ids=[rr.key_id(("width",) + k) for k in WIDTH_KEYS])
def test_row_widths_and_absent_optionals(L, m, absent):
    """Records and tails, packed and unpacked, at every row width the two formats treat differently, with every count in
    [-11, max_images] and counts beyond the row; at max_images = 100 also with color / fmin / ok handed over as NULL."""
    import torch
    c = rr.width_case(m, absent)
    n = c.n
    want_rec, want_tails = c.ref_records(), c.ref_tails()
    T = len(want_tails)
    b = _batch(n, m, _case_dev(c))
    rec = _filled(n + 2, 192)
    tails = _filled(T + 3, 392)
    assert L.hpmvs_pack_records(C.byref(b), rec.data_ptr(), None) == 0, L.hpmvs_last_error()
    assert _pack_tails(L, b, tails, T) == (0, T), L.hpmvs_last_error()
    torch.cuda.synchronize()
    assert _same(_host(rec)[:n], want_rec) and np.all(_host(rec)[n:] == FILL)
    assert _same(_host(tails)[:T], want_tails) and np.all(_host(tails)[T:] == FILL)
    # absent optionals pack as zeros, and without `ok` every long list that fits its row has a tail
    got_rec = np.frombuffer(_host(rec)[:n].tobytes(), rr.RECORD)
    for k in absent:
        assert not got_rec[k].any(), k
    nim, ok, imgs = c.col("n_images"), c.col("ok"), c.col("images")
    fits = (nim > 64) & (nim <= min(m, 256))
    assert T == int((fits if ok is None else fits & (ok != 0)).sum())

    # unpack into a sentinel-filled batch with three rows to spare; absent destinations are NULL
    d = Dst(n, m, absent)
    ob = d.batch()
    assert L.hpmvs_unpack_records(rec.data_ptr(), n, C.byref(ob), None) == 0, L.hpmvs_last_error()
    assert L.hpmvs_unpack_record_tails(tails.data_ptr(), T, 0, C.byref(ob), None) == 0, L.hpmvs_last_error()
    torch.cuda.synchronize()
    rr.unpack_tails(want_tails, 0, rr.unpack_records(want_rec, d.ref()))
    d.assert_equals_reference()
    # ... and against the input itself
    assert np.array_equal(d.got("n_images"), nim.astype(np.int16).astype(np.int32))
    got = d.got("images")
    for i in range(n):
        refined = (ok is None or ok[i] != 0) and fits[i]
        live = int(nim[i]) if refined else max(0, min(int(nim[i]), 64, m))
        assert np.array_equal(got[i, :live], imgs[i, :live]), i
        assert np.all(got[i, live:] == -1), i
    for k in ("center", "normal", "scale") + tuple(k for k in rr.OPTIONALS if k not in absent):
        assert np.array_equal(d.got(k), c.col(k)), k


def _pack_shards(L, c, cols):
    """Each non-empty shard packed on its own: (records of the round in rank order, [(lo, tails of the shard, their number)])."""
    import torch
    rec = _filled(c.n + 2, 192)
    segs = []
    for lo, hi in c.shards:
        if hi == lo:
            continue
        want = c.ref_tails(lo, hi)
        b = _batch(hi - lo, c.max_images, cols, lo)
        assert L.hpmvs_pack_records(C.byref(b), rec[lo:].data_ptr(), None) == 0, L.hpmvs_last_error()
        seg = _filled(len(want) + 2, 392)
        assert _pack_tails(L, b, seg, len(want)) == (0, len(want)), L.hpmvs_last_error()
        torch.cuda.synchronize()
        assert _same(_host(seg)[:len(want)], want) and np.all(_host(seg)[len(want):] == FILL)
        segs.append((lo, seg, len(want)))
    assert _same(_host(rec)[:c.n], c.ref_records()) and np.all(_host(rec)[c.n:] == FILL)
    return rec, segs


def test_ragged_round_composed_on_the_device(L):
    """Shards of 701, 0, 736 and 64 patches: per-shard pack, the records concatenated in rank order, ONE unpack of the
    records and one unpack of the tails per shard with its offset -- equal to the round that was never cut; then the same
    with every tail segment zero-padded to the largest and handed over with its padding."""
    import torch
    c = rr.round_case()
    n, m = c.n, c.max_images
    rec, segs = _pack_shards(L, c, _case_dev(c))
    uncut = rr.unpack_tails(c.ref_tails(), 0, rr.unpack_records(c.ref_records(), rr.sentinel_batch(n, m)))
    nim, ok = c.col("n_images"), c.col("ok")
    refined = (ok != 0) & (nim <= m)
    largest = max(t for _, _, t in segs)
    for padded in (False, True):
        d = Dst(n, m)
        ob = d.batch()
        assert L.hpmvs_unpack_records(rec.data_ptr(), n, C.byref(ob), None) == 0, L.hpmvs_last_error()
        rr.unpack_records(c.ref_records(), d.ref())
        for lo, seg, t in segs:
            if padded:
                full = torch.zeros((largest, 392), dtype=torch.uint8, device=seg.device)
                full[:t] = seg[:t]
                seg, t = full, largest
            assert L.hpmvs_unpack_record_tails(seg.data_ptr(), t, lo, C.byref(ob), None) == 0, L.hpmvs_last_error()
            rr.unpack_tails(_as_tails(seg)[:t], lo, d.ref())
        torch.cuda.synchronize()
        d.assert_equals_reference()
        for k in ("images", "n_images", "ok", "center", "normal", "scale", "color", "fmin"):
            assert np.array_equal(d.got(k), uncut[k]), (padded, k)
        assert refined.sum() > 1000 and np.array_equal(d.got("images")[refined], c.col("images")[refined])
        assert np.array_equal(d.got("n_images"), nim)


def test_offsets_that_push_tails_outside_the_batch(L):
    """A negative offset and one that puts the last tails at i >= b.n: those tails are dropped, every tail that still lands
    inside is applied, no other row changes (guard rows before and after the batch included)."""
    import torch
    c = rr.round_case()
    n, m = c.n, c.max_images
    for (lo, hi), offset in ((c.shards[0], -300), (c.shards[2], n - 400)):
        want = c.ref_tails(lo, hi)
        where = offset + want["patch"].astype(np.int64)
        inside = (where >= 0) & (where < n)
        assert inside.sum() > 20 and (~inside).sum() > 20
        d = Dst(n, m, front=400, back=800)
        assert where.min() >= -d.front and where.max() < n + 800      # (even a kernel without the check stays in the allocation)
        ob = d.batch()
        seg = _dev(_as_bytes(want, 392))
        assert L.hpmvs_unpack_record_tails(seg.data_ptr(), len(want), offset, C.byref(ob), None) == 0, L.hpmvs_last_error()
        torch.cuda.synchronize()
        rr.unpack_tails(want, offset, d.ref())
        d.assert_equals_reference()
        got = d.got("images")
        touched = np.zeros(n, bool)
        touched[where[inside]] = True
        assert np.all(got[~touched] == -7) and np.all(got[touched][:, :64] == -7)
        for t in np.nonzero(inside)[0]:
            k = int(want["count"][t])
            assert np.array_equal(got[where[t], 64:64 + k], c.col("images", lo, hi)[want["patch"][t], 64:64 + k])
            assert np.all(got[where[t], 64 + k:] == -7)


def test_malformed_tail_is_rejected_whole(L):
    """count > HPMVS_MAX_IMAGES - HPMVS_RECORD_IMAGES: the tail's row keeps its sentinels, its neighbours' tails are applied."""
    import torch
    c = rr.width_case(256)
    want = c.ref_tails().copy()
    assert len(want) > 20
    want["count"][2] = 193
    want["count"][5] = 65535
    d = Dst(c.n, c.max_images)
    ob = d.batch()
    seg = _dev(_as_bytes(want, 392))
    assert L.hpmvs_unpack_record_tails(seg.data_ptr(), len(want), 0, C.byref(ob), None) == 0, L.hpmvs_last_error()
    torch.cuda.synchronize()
    rr.unpack_tails(want, 0, d.ref())
    d.assert_equals_reference()
    got = d.got("images")
    for t in range(len(want)):
        row, k = got[want["patch"][t]], int(want["count"][t])
        if t in (2, 5):
            assert np.all(row == -7)
        else:
            assert np.array_equal(row[64:64 + k], want["images"][t, :k].astype(np.int32)) and np.all(row[64 + k:] == -7)


def test_exchange_on_a_stream_behind_the_kernels_that_produce_its_inputs(L):
    """pack -> tails -> unpack on a torch stream whose handle is passed as `stream`, enqueued behind the kernels that write
    n_images and images on that stream, with no synchronise but the one hpmvs_pack_record_tails documents: the same bytes
    as on the null stream."""
    import torch
    c = rr.round_case()
    n, m = c.n, c.max_images
    want_rec, want_tails = c.ref_records(), c.ref_tails()
    T = len(want_tails)
    cols = _case_dev(c)

    def run(cols, stream, produce=None):
        rec, tails, d = _filled(n + 2, 192), _filled(T + 3, 392), Dst(n, m)
        torch.cuda.synchronize()
        if produce is not None:
            produce()
        b, ob = _batch(n, m, cols), d.batch()
        assert L.hpmvs_pack_records(C.byref(b), rec.data_ptr(), stream) == 0, L.hpmvs_last_error()
        assert _pack_tails(L, b, tails, T, stream) == (0, T), L.hpmvs_last_error()
        assert L.hpmvs_unpack_records(rec.data_ptr(), n, C.byref(ob), stream) == 0, L.hpmvs_last_error()
        assert L.hpmvs_unpack_record_tails(tails.data_ptr(), T, 0, C.byref(ob), stream) == 0, L.hpmvs_last_error()
        return rec, tails, d

    rec0, tails0, d0 = run(cols, None)
    torch.cuda.synchronize()
    assert _same(_host(rec0)[:n], want_rec) and _same(_host(tails0)[:T], want_tails)

    # the inputs exist only in a disguised form until kernels on the stream write them, behind a few matrix products
    s = torch.cuda.Stream()
    hidden_n, hidden_i = cols["n_images"] - 1000, cols["images"] ^ 0x5555
    staged = dict(cols, n_images=torch.full_like(cols["n_images"], -1), images=torch.full_like(cols["images"], -7))
    work = torch.ones((2048, 2048), device=hidden_n.device)

    def produce():
        with torch.cuda.stream(s):
            x = work
            for _ in range(8):
                x = (x @ work) * 1e-4
            torch.add(hidden_n, 1000, out=staged["n_images"])
            torch.bitwise_xor(hidden_i, 0x5555, out=staged["images"])

    rec1, tails1, d1 = run(staged, C.c_void_p(s.cuda_stream), produce)
    s.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(rec1, rec0) and torch.equal(tails1, tails0)
    for k in d0.dev:
        assert torch.equal(d1.dev[k], d0.dev[k]), k
    rr.unpack_tails(want_tails, 0, rr.unpack_records(want_rec, d1.ref()))
    d1.assert_equals_reference()
