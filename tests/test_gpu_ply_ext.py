"""The patch cloud as the reference's extended PLY file on the GPU (kernel_ply.hip behind hpmvs_ply_ext_batch / api.ply_ext):
every file equals, byte for byte, the one tests/ply_ref.py builds with Python formatting -- the pin tests/test_cpu_ply_text.py
states: this machine's C library, never the code under test and never a file of the reference's own (its translation units
cannot be compiled where the fixtures are made).  Row counts straddle the wavefront (64 rows) and workgroup (256 rows)
boundaries of the staged copy; line lengths run from the shortest line there is to the longest (104 bytes: seven
12-character floats and three 3-digit colours -- the colours are bytes, so no line reaches ten floats' 143), so that every
wavefront's block starts at an arbitrary byte offset."""
import ctypes as C

import numpy as np
import pytest

import ply_ref as ref

pytestmark = pytest.mark.gpu
ROW_COUNTS = (0, 1, 63, 64, 65, 128, 4097)
SENTINEL = 0xA5
ERR_ARG = -2


@pytest.fixture(scope="module")
def api():
    from hpmvs_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device: -m gpu tests need the MI355X box (no CPU fallback exists)")
    return api


def make_batch(api, rows):
    b = api.Batch(rows.center, rows.normal, rows.scale, rows.n_images, rows.images)
    b.color[...] = rows.color
    return b


@pytest.fixture(scope="module")
def cases(api):
    """row count -> (the rows, their batch), made once"""
    out = {}
    for n in ROW_COUNTS:
        rows = ref.Rows(n, max_images=64, seed=100 + n)
        out[n] = (rows, make_batch(api, rows))
    return out


def raw_call(api, b, order, n_rows, flags, out, cap, on_device=0):
    n = C.c_size_t(0)
    rc = api.lib().hpmvs_ply_ext_batch(0, C.byref(b), api._ptr(order), n_rows, flags, None if out is None else out.ctypes.data, cap,
                                       C.byref(n), on_device, None)
    return rc, n.value, api.lib().hpmvs_last_error().decode()


def flag_kwargs(flags):
    return dict(binary=bool(flags & 1), normal=bool(flags & 2), scale=bool(flags & 4), visibility=bool(flags & 8))


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("binary", (False, True))
def test_row_counts(api, cases, n, binary):
    rows, batch = cases[n]
    flags = 14 | int(binary)
    got = api.ply_ext(batch, **flag_kwargs(flags)).tobytes()
    assert got == ref.build(rows, None, flags)


def test_line_lengths_cover_both_ends(cases):
    body = ref.build(cases[65][0], None, 6).split(b"end_header\n", 1)[1]
    lens = [len(l) + 1 for l in body.split(b"\n")[:-1]]
    assert min(lens) == 21 and max(lens) == 104 and len(set(lens)) > 20


@pytest.mark.parametrize("flags", range(16))
def test_every_flag_set(api, cases, flags):
    rows, batch = cases[65]
    assert api.ply_ext(batch, **flag_kwargs(flags)).tobytes() == ref.build(rows, None, flags)


@pytest.mark.parametrize("binary", (False, True))
def test_order(api, cases, binary):
    rows, batch = cases[128]
    rng = np.random.default_rng(5)
    flags = 14 | int(binary)
    for order in (rng.permutation(128), rng.integers(0, 128, 200), np.array([1, 1, 0, 127, 1]), np.arange(70)[::-1], np.zeros(0, np.int64)):
        assert api.ply_ext(batch, order=order, **flag_kwargs(flags)).tobytes() == ref.build(rows, order, flags)


def test_bad_rows_are_named_and_write_nothing(api, cases):
    rows, batch = cases[128]
    b = batch.c_struct()
    out = np.full(1 << 16, SENTINEL, np.uint8)
    order = np.arange(100, dtype=np.int32)
    for bad in (128, -1):
        order[37] = bad
        order[80] = bad
        rc, _, msg = raw_call(api, b, order, 100, 14, out, out.nbytes)
        assert rc == ERR_ARG and "row 37 " in msg, msg
        assert (out == SENTINEL).all()
    with pytest.raises(api.HpmvsError, match="row 37 "):
        api.ply_ext(batch, order=order)
    saved = batch.n_images[41]
    batch.n_images[41] = batch.max_images + 1
    try:
        rc, _, msg = raw_call(api, b, None, 0, 14, out, out.nbytes)
        assert rc == ERR_ARG and "row 41 " in msg and "n_images" in msg, msg
        assert (out == SENTINEL).all()
        batch.n_images[41] = -1
        rc, _, msg = raw_call(api, b, None, 0, 15, out, out.nbytes)
        assert rc == ERR_ARG and "row 41 " in msg, msg
        assert (out == SENTINEL).all()
    finally:
        batch.n_images[41] = saved


@pytest.mark.parametrize("flags", (14, 15, 6))
def test_size_contract(api, cases, flags):
    rows, batch = cases[65]
    want = ref.build(rows, None, flags)
    b = batch.c_struct()
    rc, n, msg = raw_call(api, b, None, 0, flags, None, 0)
    assert rc == 0 and n == len(want), msg
    out = np.full(n + 256, SENTINEL, np.uint8)
    rc, n2, msg = raw_call(api, b, None, 0, flags, out, n - 1)
    assert rc == ERR_ARG and n2 == n and (out == SENTINEL).all(), msg
    rc, n3, msg = raw_call(api, b, None, 0, flags, out, out.nbytes)
    assert rc == 0 and n3 == n, msg
    assert out[:n].tobytes() == want and (out[n:] == SENTINEL).all()   # the bytes past *n keep the sentinel


@pytest.mark.parametrize("flags", (14, 15))
def test_device_pointers_give_the_same_bytes(api, cases, flags):
    import torch
    rows, batch = cases[4097]
    dev = api.Batch(rows.center, rows.normal, rows.scale, rows.n_images, rows.images)
    for name in ("center", "normal", "scale", "n_images", "images"):
        setattr(dev, name, torch.from_numpy(getattr(batch, name)).to("cuda:0"))
    dev.color = torch.from_numpy(batch.color).to("cuda:0")
    order = np.random.default_rng(9).permutation(4097)[:1000].astype(np.int32)
    want = ref.build(rows, None, flags)
    assert api.ply_ext(dev, **flag_kwargs(flags)).tobytes() == want
    got = api.ply_ext(dev, order=torch.from_numpy(order).to("cuda:0"), **flag_kwargs(flags)).tobytes()
    assert got == ref.build(rows, order, flags)
    stream = torch.cuda.Stream()   # ... and on a stream of the caller's
    b, n = dev.c_struct(), C.c_size_t(0)
    out = np.full(len(want) + 64, SENTINEL, np.uint8)
    rc = api.lib().hpmvs_ply_ext_batch(0, C.byref(b), None, 0, flags, out.ctypes.data, out.nbytes, C.byref(n), 1, C.c_void_p(stream.cuda_stream))
    assert rc == 0 and out[:n.value].tobytes() == want and (out[n.value:] == SENTINEL).all()


def test_a_refined_cloud(api, tmp_path):
    """3 views of 640 x 480, 96 seeds refined as smoke() refines them; the rows with ok, in order"""
    from hpmvs_amd import synth
    syn = synth.make_scene(3, 640, 480, n_waves=16)
    seeds = synth.make_seeds(syn, 96, start_level=2)
    scene = api.Scene(syn, device=0)
    try:
        batch = api.Batch.from_seeds(seeds)
        api.optimize_batch(scene, batch)
    finally:
        scene.close()
    order = np.nonzero(batch.ok)[0]
    assert len(order) >= 10
    text = api.ply_ext(batch, order=order).tobytes()
    assert text == ref.build(batch, order, 14)
    path = tmp_path / "patches.ply"
    assert api.write_ext_ply(str(path), batch, order=order, binary=True) == path.stat().st_size
    data = path.read_bytes()
    assert data == ref.build(batch, order, 15)
    # ... and the binary file parses back field by field
    head, body = data.split(b"end_header\n", 1)
    assert f"element vertex {len(order)}".encode() in head
    vert = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3), ("scale", "<f4")])
    assert vert.itemsize == 31
    v = np.frombuffer(body, dtype=vert, count=len(order))
    assert (v["xyz"] == batch.center[order, :3]).all() and (v["n"] == batch.normal[order, :3]).all()
    assert (v["rgb"] == np.clip(np.trunc(batch.color[order]), 0, 255).astype(np.uint8)).all() and (v["scale"] == batch.scale[order]).all()
    at = 31 * len(order)
    for p in order:
        n = int(np.frombuffer(body, "<u4", 1, at)[0])
        assert n == batch.n_images[p]
        assert (np.frombuffer(body, "<u4", n, at + 4) == batch.images[p, :n].astype(np.uint32)).all()
        at += 4 + 4 * n
    assert at == len(body)
