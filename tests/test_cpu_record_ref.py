"""The per-round exchange's two wire formats on the CPU: every case of tests/record_ref.py goes through the reference
(a reading of include/hpmvs_amd.h alone) and through hpmvs_amd.distributed, and the bytes and the unpacked arrays are
compared.  The cases' preconditions are asserted here too, so that what tests/test_gpu_record_exchange.py relies on (tails
beyond the scan's first 256-block chunk, empty runs, full blocks, a shard without tails ...) is verified without a GPU."""
import numpy as np
import pytest
import torch

import record_ref as rr
from hpmvs_amd import distributed as dd

KEYS = rr.case_keys()
t = torch.from_numpy


def _bytes(a, width):
    return t(np.frombuffer(a.tobytes(), np.uint8).reshape(-1, width).copy())


_sentinel_batch = rr.sentinel_batch


def _py_pack(c, lo=0, hi=None):
    """hpmvs_amd.distributed's records and tails of rows [lo, hi); absent optionals go in as the zeros the header prescribes."""
    hi = c.n if hi is None else hi
    n = hi - lo
    col = lambda k: c.col(k, lo, hi)
    color = col("color") if col("color") is not None else np.zeros((n, 3), np.float32)
    fmin = col("fmin") if col("fmin") is not None else np.zeros(n)
    ok = col("ok") if col("ok") is not None else np.zeros(n, np.uint8)
    refused = n > 0 and int(col("n_images").max()) > c.max_images    # counts the checker refuses
    rec = dd.pack_records(t(col("center")), t(col("normal")), t(color), t(col("scale")), t(fmin), t(ok), t(col("n_images")),
                          t(col("images")), check=not refused)
    tails = dd.pack_tails(None if col("ok") is None else t(col("ok")), t(col("n_images")), t(col("images")))
    return rec, tails


def test_layouts_are_the_headers():
    assert rr.RECORD.itemsize == 192 == dd.RECORD_BYTES and rr.TAIL.itemsize == 392 == dd.TAIL_BYTES
    off = lambda d: {k: d.fields[k][1] for k in d.names}
    assert off(rr.RECORD) == dict(center=0, normal=16, color=32, scale=44, fmin=48, ok=56, pad0=57, n_images=58, pad1=60, images=64)
    assert off(rr.TAIL) == dict(patch=0, count=4, pad=6, images=8)
    assert rr.RECORD["images"].shape == (64,) and rr.TAIL["images"].shape == (192,)


@pytest.mark.parametrize("key", KEYS, ids=rr.key_id)
def test_case_preconditions(key):
    c = rr.case(key)
    n, m = c.n, c.max_images
    tails = c.ref_tails()
    patch = tails["patch"].astype(np.int64)
    assert np.all(np.diff(patch) > 0)
    if c.expect == "many":
        assert len(tails) > 20, len(tails)
    elif c.expect == "one":
        assert len(tails) == 1
    elif c.expect == "zero":
        assert len(tails) == 0
    nim = c.arrays["n_images"]
    if key[0] == "scan":
        past = slice(n, None)
        assert len(nim) >= n + 64 and np.all(nim[past] > 64) and np.all(nim[past] <= m) and np.all(c.arrays["ok"][past] == 1)
        if key[2] == "c":
            assert len(tails) == n
        if key[2] == "d":
            nb = (n + 63) // 64
            assert np.all(patch >= (nb - 1) * 64) and patch[-1] == n - 1
        if key[2] == "b":
            assert np.all(patch >= 256 * 64)
    if key[0] == "scan" and key[1:] in rr.SCAN_CARRY:
        nb = (n + 63) // 64
        per_block = np.bincount(patch // 64, minlength=nb)
        assert int((patch // 64 >= 256).sum()) >= 50
        assert np.any(per_block == 64)
        empty = per_block == 0
        assert np.any(empty[:-2] & empty[1:-1] & empty[2:])
        assert nb > 256
    if key[0] == "width":
        have = set(int(v) for v in nim[:n])
        assert have >= set(range(-11, m + 1))
        assert any(v > m for v in have) and 300 in have
        for v in (64, 65, 256):
            assert v > m or v in have
        assert n == 130 or (m >= 255 and n == 300)
        if m > 64:
            ids = tails["images"][tails["images"] != rr.NO_IMAGE]
            assert ids.max() == 65534 and np.any(ids >= 32768) and np.any(ids < 32768)
            assert int(tails["count"].max()) == m - 64 and int(tails["count"].min()) == 1
            ok = c.col("ok")
            if ok is not None:   # long lists that were not refined travel without a tail
                assert np.any((nim[:n] > 64) & (nim[:n] <= m) & (ok == 0))
        else:
            assert len(tails) == 0
    if key[0] == "round":
        assert [hi - lo for lo, hi in c.shards] == [701, 0, 736, 64] and c.shards[-1][1] == n == 1501 and m == 96
        per_shard = [len(c.ref_tails(lo, hi)) for lo, hi in c.shards if hi > lo]
        assert sorted(v == 0 for v in per_shard) == [False, False, True]
        assert all(v > 20 for v in per_shard if v)
        lo = c.shards[-1][0]
        assert np.any(nim[lo:] > 64)   # the shard without tails has long lists, none of them refined


@pytest.mark.parametrize("key", KEYS, ids=rr.key_id)
def test_python_codec_writes_the_reference_bytes(key):
    c = rr.case(key)
    n, m = c.n, c.max_images
    want_tails = c.ref_tails()
    if n > 2000:
        # (the big scan cases are about the tail list; their records are not packed one id at a time in Python)
        got = dd.pack_tails(t(c.col("ok")), t(c.col("n_images")), t(c.col("images")))
        assert got.numpy().tobytes() == want_tails.tobytes()
        return
    want_rec = c.ref_records()
    rec, tails = _py_pack(c)
    assert rec.numpy().tobytes() == want_rec.tobytes()
    assert tails.numpy().tobytes() == want_tails.tobytes()
    # unpack: the reference into a sentinel-filled batch, distributed.py into fresh arrays
    ref = rr.unpack_tails(want_tails, 0, rr.unpack_records(want_rec, _sentinel_batch(n, m, c.absent)))
    u = dd.unpack_records(_bytes(want_rec, 192), _bytes(want_tails, 392))
    for k in ("center", "normal", "scale", "n_images"):
        assert np.array_equal(u[k], ref[k]), k
    # what the record carries for an absent optional is the header's zero
    zero = dict(color=np.zeros((n, 3), np.float32), fmin=np.zeros(n), ok=np.zeros(n, np.uint8))
    for k in rr.OPTIONALS:
        want = zero[k] if k in c.absent else ref[k]
        assert np.array_equal(u[k], want.astype(bool) if k == "ok" else want), k
        assert ref[k] is None or np.array_equal(ref[k], c.col(k))
    w = min(m, u["images"].shape[1])
    assert np.array_equal(u["images"][:, :w], ref["images"][:, :w])
    assert np.all(u["images"][:, w:] == -1) and np.all(ref["images"][:, w:] == -1)
    # and against the input itself: the signed 16-bit count, every refined list in full, -1 elsewhere
    nim = c.col("n_images")
    assert np.array_equal(ref["n_images"], nim.astype(np.int16).astype(np.int32))
    ok = c.col("ok")
    for i in range(n):
        whole = (ok is None or ok[i]) and nim[i] <= min(m, 256)
        live = max(0, min(int(nim[i]), m) if whole else min(int(nim[i]), 64, m))
        assert np.array_equal(ref["images"][i, :live], c.col("images")[i, :live]), i
        assert np.all(ref["images"][i, live:] == -1), i


def test_python_round_of_ragged_shards_equals_the_uncut_round():
    c = rr.round_case()
    n, m = c.n, c.max_images
    recs, tails, ref = [], [], _sentinel_batch(n, m)
    for lo, hi in c.shards:
        if hi == lo:
            continue
        r, tl = _py_pack(c, lo, hi)
        assert r.numpy().tobytes() == c.ref_records(lo, hi).tobytes() and tl.numpy().tobytes() == c.ref_tails(lo, hi).tobytes()
        recs.append(r)
        tl = tl.clone()
        tl[:, 0:4] = (tl[:, 0:4].contiguous().view(torch.int32) + lo).view(torch.uint8)   # shard index -> round index
        tails.append(tl)
    rec = torch.cat(recs)
    assert rec.numpy().tobytes() == c.ref_records().tobytes()
    rr.unpack_records(c.ref_records(), ref)
    for lo, hi in c.shards:
        rr.unpack_tails(c.ref_tails(lo, hi), lo, ref)
    uncut = rr.unpack_tails(c.ref_tails(), 0, rr.unpack_records(c.ref_records(), _sentinel_batch(n, m)))
    u = dd.unpack_records(rec, torch.cat(tails))
    assert np.array_equal(ref["images"], uncut["images"])
    assert np.array_equal(u["images"], ref["images"][:, :u["images"].shape[1]]) and np.all(ref["images"][:, u["images"].shape[1]:] == -1)
    refined = (c.col("ok") != 0) & (c.col("n_images") <= m)
    assert refined.sum() > 1000 and np.array_equal(ref["images"][refined], c.col("images")[refined])


@pytest.mark.parametrize("count", [193, 40000, 65535])
def test_python_unpack_refuses_a_malformed_tail(count):
    c = rr.width_case(100)
    rec, tails = c.ref_records(), c.ref_tails().copy()
    assert len(tails) > 3
    dd.unpack_records(_bytes(rec, 192), _bytes(tails, 392))
    tails["count"][2] = 192      # the most a tail holds: taken
    u = dd.unpack_records(_bytes(rec, 192), _bytes(tails, 392))
    assert u["images"].shape[1] == 256
    tails["count"][2] = count
    with pytest.raises(ValueError, match="malformed tail 2"):
        dd.unpack_records(_bytes(rec, 192), _bytes(tails, 392))


def test_reference_drops_and_rejects_as_the_header_says():
    """The reference's own edge rules (the GPU test compares the kernels with them): an all-zero tail is a no-op, a tail
    outside the batch is dropped, a malformed one is rejected whole."""
    b = dict(images=np.full((5, 80), -7, np.int32))
    tl = np.zeros(4, rr.TAIL)
    tl["patch"][1:] = (3, 4, 1)
    tl["count"][1:] = (2, 3, 193)
    tl["images"][:] = 9
    rr.unpack_tails(tl, 1, b, n=5)       # -> rows 1 (count 0), 4, 5 (outside), 2 (malformed)
    want = np.full((5, 80), -7, np.int32)
    want[4, 64:66] = 9
    assert np.array_equal(b["images"], want)
    rr.unpack_tails(tl, -4, b, n=5)      # -> rows -4, -1, 0, -3
    want[0, 64:67] = 9
    assert np.array_equal(b["images"], want)
