"""The two forms of one batch entry point agree: host arrays (on_device = 0, through hpmvs_amd.api) and device pointers
on a caller's stream (on_device = 1, through api.lib(); torch is only the allocator and the stream here).  Every output
array byte for byte.  What "right" means is the host-pointer form, which the oracle tests establish; a device-pointer
call leaves untouched what its kernel does not write where a staged call returns 0 (include/hpmvs_amd.h), so the device
outputs start as zeros."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RESET_DEPTH = np.float32(1000.0)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def refined(tiny_scene, gpu_scene):
    """A refined batch with both kinds of patches (the seeds of test_gpu_zero_copy.py)."""
    from hpmvs_amd import api, synth
    seeds = synth.make_seeds(tiny_scene, 20000, start_level=2, max_images=16)
    b = api.Batch.from_seeds(seeds)
    api.optimize_batch(gpu_scene, b)
    assert 0 < b.ok.sum() < b.n
    return b


class OnDevice:
    """Device copies of a host Batch's fourteen arrays, a PatchBatch of their pointers, and a stream of its own."""

    def __init__(self, batch):
        import torch
        from hpmvs_amd import api
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k))).to(self.dev) for k in api.Batch.FIELDS}
        self.pb = api.PatchBatch()
        self.pb.n, self.pb.max_images = batch.n, batch.max_images
        for k, v in self.t.items():
            setattr(self.pb, k, v.data_ptr())
        self.stream = torch.cuda.Stream(device=self.dev)
        self.keep = []

    def zeros(self, shape, dtype):
        z = self.torch.zeros(shape, dtype=dtype, device=self.dev)
        self.keep.append(z)
        return z

    def upload(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def call(self, fn, *args):
        """fn(*args, on_device = 1, stream) behind the uploads, then wait for the stream."""
        from hpmvs_amd import api
        self.stream.wait_stream(self.torch.cuda.current_stream(self.dev))  # the uploads ran on the current stream
        with self.torch.cuda.stream(self.stream):
            rc = fn(*args, 1, C.c_void_p(self.stream.cuda_stream))
        assert rc == 0, api.lib().hpmvs_last_error()
        self.stream.synchronize()


def all_depth_levels(scene):
    from hpmvs_amd import api
    out = []
    for view in range(scene.n_views):
        level = 0
        while True:
            try:
                out.append(api.depth_level(scene, view, level))
            except api.HpmvsError:
                break
            level += 1
        assert level > 0
    return out


def test_init_patches_batch(tiny_scene, gpu_scene):
    from hpmvs_amd import api, synth
    xyz, off, img = synth.make_nvm_points(tiny_scene, 400, start_level=2, noise=1.5)
    want = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2)
    assert 0 < want.ok.sum() < want.n
    n, m = want.n, want.max_images
    blank = api.Batch(np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32),
                      np.zeros(n, np.int32), np.zeros((n, m), np.int32))
    d = OnDevice(blank)
    dxyz = d.upload(np.asarray(xyz, np.float64))
    doff, dimg = d.upload(np.asarray(off, np.int32)), d.upload(np.asarray(img, np.int32))
    o = api.default_options()
    d.call(api.lib().hpmvs_init_patches_batch, gpu_scene.h, C.byref(o), 2, n, dxyz.data_ptr(), doff.data_ptr(),
           dimg.data_ptr(), C.byref(d.pb))
    for k in api.Batch.FIELDS:
        assert same_bytes(d.t[k].cpu().numpy(), getattr(want, k)), k


def test_objective_batch(gpu_scene, refined):
    import torch
    from hpmvs_amd import api
    f, g = api.objective_batch(gpu_scene, refined, refined.x)
    assert g.any()
    d = OnDevice(refined)
    dx = d.upload(refined.x)
    df, dg = d.zeros(refined.n, torch.float64), d.zeros(refined.n, torch.int32)
    o = api.default_options()
    d.call(api.lib().hpmvs_objective_batch, gpu_scene.h, C.byref(o), C.byref(d.pb), dx.data_ptr(), df.data_ptr(),
           dg.data_ptr())
    assert same_bytes(df.cpu().numpy(), f)
    assert same_bytes(dg.cpu().numpy(), g)


def test_inccs_batch(gpu_scene, refined):
    import torch
    from hpmvs_amd import api
    want = api.inccs_batch(gpu_scene, refined, 0, 1)
    assert want.any()
    d = OnDevice(refined)
    dout = d.zeros((refined.n, refined.max_images), torch.float32)
    o = api.default_options()
    d.call(api.lib().hpmvs_inccs_batch, gpu_scene.h, C.byref(o), C.byref(d.pb), 0, 1, dout.data_ptr())
    assert same_bytes(dout.cpu().numpy(), want)


def test_level_support_batch(gpu_scene, refined):
    import torch
    from hpmvs_amd import api
    want = api.level_support_batch(gpu_scene, refined, 0)
    assert want.any()
    d = OnDevice(refined)
    dsup = d.zeros(refined.n, torch.int32)
    d.call(api.lib().hpmvs_level_support_batch, gpu_scene.h, C.byref(d.pb), 0, dsup.data_ptr())
    assert same_bytes(dsup.cpu().numpy(), want)


def test_set_depths_batch(gpu_scene, refined):
    from hpmvs_amd import api
    api.depth_reset(gpu_scene)
    api.set_depths_batch(gpu_scene, refined)
    want = all_depth_levels(gpu_scene)
    assert any((lv != RESET_DEPTH).any() for lv in want)
    api.depth_reset(gpu_scene)
    assert all((lv == RESET_DEPTH).all() for lv in all_depth_levels(gpu_scene))
    d = OnDevice(refined)
    d.call(api.lib().hpmvs_set_depths_batch, gpu_scene.h, C.byref(d.pb))
    got = all_depth_levels(gpu_scene)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bytes(a, b), k


def test_depth_ops_batch_with_subtractions(gpu_scene, refined):
    """Every patch recorded first (the host form of set_depths, for both runs), then the batch replayed in order with every
    third recorded patch taken out again."""
    from hpmvs_amd import api
    ok = refined.ok.astype(bool)
    sub = (np.arange(refined.n) % 3 == 0).astype(np.uint8)
    assert 0 < sub[ok].sum() < ok.sum()   # both set and subtract entries among the patches that count

    def prelude():
        api.depth_reset(gpu_scene)
        api.set_depths_batch(gpu_scene, refined)
        return all_depth_levels(gpu_scene)

    before = prelude()
    api.depth_ops_batch(gpu_scene, refined, sub)
    want = all_depth_levels(gpu_scene)
    assert any(not same_bytes(a, b) for a, b in zip(want, before))   # the subtractions changed the maps
    prelude()
    d = OnDevice(refined)
    dsub = d.upload(sub)
    d.call(api.lib().hpmvs_depth_ops_batch, gpu_scene.h, C.byref(d.pb), dsub.data_ptr())
    got = all_depth_levels(gpu_scene)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bytes(a, b), k


def recorded_half(gpu_scene, refined):
    """Depth maps holding the first half of the refined patches: the gates then see written and empty cells."""
    from hpmvs_amd import api
    first = api.Batch(refined.center, refined.normal, refined.scale, refined.n_images, refined.images)
    first.ok[:] = refined.ok * (np.arange(refined.n) < refined.n // 2)
    api.depth_reset(gpu_scene)
    api.set_depths_batch(gpu_scene, first)


def test_depth_gates_batch(gpu_scene, refined):
    import torch
    from hpmvs_amd import api
    recorded_half(gpu_scene, refined)
    want = api.depth_gates_batch(gpu_scene, refined, 1.0, 0)
    assert any(w.any() for w in want)   # the counts are not all zero
    d = OnDevice(refined)
    outs = [d.zeros(refined.n, torch.int32) for _ in range(3)]
    d.call(api.lib().hpmvs_depth_gates_batch, gpu_scene.h, C.byref(d.pb), C.c_float(1.0), 0, *[t.data_ptr() for t in outs])
    for k, (t, w) in enumerate(zip(outs, want)):
        assert same_bytes(t.cpu().numpy(), w), k


def test_depth_footprints_batch(gpu_scene, refined):
    import torch
    from hpmvs_amd import api
    recorded_half(gpu_scene, refined)
    want = api.depth_footprints_batch(gpu_scene, refined)
    assert any(w.any() for w in want)   # the footprints are not all zero
    d = OnDevice(refined)
    outs = [d.zeros(w.shape, torch.int32) for w in want]
    d.call(api.lib().hpmvs_depth_footprints_batch, gpu_scene.h, C.byref(d.pb), *[t.data_ptr() for t in outs])
    for k, (t, w) in enumerate(zip(outs, want)):
        assert same_bytes(t.cpu().numpy(), w), k
