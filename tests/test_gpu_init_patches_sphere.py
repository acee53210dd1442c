"""The scene-centre gate of --only_sphere on the device: hpmvs_init_patches_sphere_batch / api.init_patches_batch(sphere=...).

The yardstick for the gate is tests/scene_center_ref.py (numpy float64, Scene.cpp:118-121): given (centre, radius) the gate is
exact, so there are no tolerances here.  For everything behind the gate the yardstick is the oracle on the surviving points: the
reference's gate is a `continue` in front of the loop body, so its result with the gate is its result on the kept subset."""
import ctypes as C
import itertools

import numpy as np
import pytest

import scene_center_ref as ref
from test_gpu_device_pointers import OnDevice, same_bytes

pytestmark = pytest.mark.gpu

ERR_ARG = -2


def assert_gated_rows(batch, xyz, rows):
    """a gated row is a row rejected before optimize(): ok 0, n_images 0, centre (float)xyz with w = 1, normal 0, scale 0"""
    rows = np.asarray(rows)
    assert np.array_equal(batch.stage[rows], np.full(len(rows), 13, np.int32))
    assert not batch.ok[rows].any() and not batch.n_images[rows].any()
    with np.errstate(over="ignore"):
        want = np.concatenate([np.asarray(xyz, np.float64)[rows].astype(np.float32), np.ones((len(rows), 1), np.float32)], axis=1)
    assert same_bytes(batch.center[rows], want)
    assert not batch.normal[rows].any() and not batch.scale[rows].any()


def crafted_points():
    """~300 points around the sphere (1, 2, 3; 5): exactly on it (3-4-5 offsets, every sign), the same offsets scaled by
    1 +- 2^-40, far inside, far outside, one +inf and one NaN coordinate.  Returns xyz and the index ranges."""
    c = np.array([1.0, 2.0, 3.0])
    offs = []
    for base in ((3.0, 4.0, 0.0), (0.0, 3.0, 4.0), (4.0, 0.0, 3.0)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            o = tuple(b * s for b, s in zip(base, sg))
            if o not in offs:
                offs.append(o)
    offs = np.array(offs)
    assert len(offs) == 12
    on = c + offs
    assert np.array_equal(on - c, offs)  # exact in float64: the distance is exactly 5
    near = np.concatenate([c + offs * (1.0 + 2.0 ** -40), c + offs * (1.0 - 2.0 ** -40)])
    rng = np.random.Generator(np.random.PCG64(1305))
    d = rng.normal(size=(260, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = c + d[:130] * rng.uniform(0.0, 3.0, size=(130, 1))
    outside = c + d[130:] * rng.uniform(8.0, 50.0, size=(130, 1))
    special = np.array([[1.0, np.inf, 3.0], [1.0, 2.0, np.nan]])
    xyz = np.concatenate([on, near, inside, outside, special])
    k = np.cumsum([0, len(on), len(near), len(inside), len(outside), len(special)])
    return xyz, {"on": range(k[0], k[1]), "near": range(k[1], k[2]), "inside": range(k[2], k[3]), "outside": range(k[3], k[4]),
                 "inf": k[4], "nan": k[4] + 1}


def test_gate_is_exact(gpu_scene):
    from hpmvs_amd import api
    sphere = (1.0, 2.0, 3.0, 5.0)
    xyz, where = crafted_points()
    n = len(xyz)
    off = (3 * np.arange(n + 1)).astype(np.int32)
    img = np.tile(np.arange(3, dtype=np.int32), n)
    gated = ref.gate(xyz, sphere)
    # what the inputs are for, asserted on the restatement alone
    assert not gated[list(where["on"])].any() and not gated[list(where["inside"])].any() and gated[list(where["outside"])].all()
    near = gated[list(where["near"])]
    assert near[:12].all() and not near[12:].any()  # both outcomes within 2^-40 of the surface
    assert gated[where["inf"]] and not gated[where["nan"]]
    plain = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2)
    got = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, sphere=sphere)
    assert not (plain.stage == 13).any()
    assert np.array_equal(got.stage == 13, gated), np.nonzero((got.stage == 13) != gated)[0]
    assert_gated_rows(got, xyz, np.nonzero(gated)[0])
    keep = np.nonzero(~gated)[0]
    for k in api.Batch.FIELDS:
        assert same_bytes(getattr(got, k)[keep], getattr(plain, k)[keep]), k
    print("gate:", n, "points,", int(gated.sum()), "gated; kept stages", np.unique(got.stage[keep], return_counts=True))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sphere_comes_before_the_measurement_count(gpu_scene, n):
    """points alternately inside and outside, none with a measurement: stages alternate 10 / 13, across the 256-thread blocks"""
    from hpmvs_amd import api
    xyz = np.zeros((n, 3))
    xyz[1::2, 0] = 7.0
    xyz[:, 2] = np.arange(n) * 1e-3
    off = np.zeros(n + 1, np.int32)
    got = api.init_patches_batch(gpu_scene, xyz, off, np.zeros(0, np.int32), start_level=2, sphere=(0.0, 0.0, 0.0, 5.0))
    want = np.where(np.arange(n) % 2 == 1, 13, 10).astype(np.int32)
    assert np.array_equal(want == 13, ref.gate(xyz, (0.0, 0.0, 0.0, 5.0)))
    assert np.array_equal(got.stage, want)
    assert not got.ok.any() and not got.n_images.any() and not got.normal.any() and not got.scale.any()
    assert same_bytes(got.center, np.concatenate([xyz.astype(np.float32), np.ones((n, 1), np.float32)], axis=1))


def test_parity_behind_the_gate(tiny_scene, oracle_scene, gpu_scene):
    """configs[0], 400 NVM points, sphere (0, 0, 0; 5): 123 inside (61 refine), 277 outside, which un-gated would end at stages
    0, 2, 10 and 12 -- stage 13 overrides each.  Kept rows against the oracle on the kept subset, compared as
    test_gpu_optimize.py::test_init_patches_batch_matches_oracle compares them."""
    from hpmvs_amd import api, synth
    from oracle import oracle as orc
    sphere = (0.0, 0.0, 0.0, 5.0)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 400, start_level=2, noise=1.5)
    gated = ref.gate(xyz, sphere)
    keep = np.nonzero(~gated)[0]
    counts = np.diff(off)
    assert (counts[gated] < 3).any()  # a gated point that stage 10 would have taken
    batch = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, sphere=sphere)
    assert np.array_equal(batch.stage == 13, gated)
    assert_gated_rows(batch, xyz, np.nonzero(gated)[0])
    # the kept subset as a model of its own
    koff = np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int32)
    kimg = np.concatenate([img[off[k]:off[k + 1]] for k in keep]).astype(np.int32)
    P = orc.init_patches(oracle_scene, xyz[keep], koff, kimg, start_level=2, n_threads=8)
    st_cpu = np.array([p.stage for p in P])
    assert (st_cpu == 0).sum() >= 50
    assert np.array_equal(st_cpu, batch.stage[keep]), np.nonzero(st_cpu != batch.stage[keep])[0][:10]
    assert np.array_equal(st_cpu == 0, batch.ok[keep].astype(bool))
    for j, k in enumerate(keep):
        p = P[j]
        assert np.array_equal(np.array(p.center[:], dtype=np.float32), batch.center[k]), k
        if p.stage < 10:  # seed was built: normal/scale/images defined
            assert np.float32(p.scale) == batch.scale[k]
            if p.stage == 0 or p.stage == 12:
                assert np.array_equal(np.array(p.normal[:], dtype=np.float32), batch.normal[k]), k
                assert list(p.images[:p.n_images]) == list(batch.images[k, :batch.n_images[k]])
    print("parity:", len(keep), "kept,", int((st_cpu == 0).sum()), "refined,", int(gated.sum()), "gated")


def test_forms_and_errors(tiny_scene, gpu_scene):
    from hpmvs_amd import api, synth
    sphere = (0.0, 0.0, 0.0, 5.0)
    xyz, off, img = synth.make_nvm_points(tiny_scene, 400, start_level=2, noise=1.5)
    want = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, sphere=sphere)
    plain = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2)
    assert 0 < (want.stage == 13).sum() < want.n and 0 < want.ok.sum()
    n, m = want.n, want.max_images
    o = api.default_options()
    L = api.lib()

    def blank():
        return api.Batch(np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32),
                         np.zeros(n, np.int32), np.zeros((n, m), np.int32))

    # device-pointer arrays (the sphere stays a host pointer) give the host form's bytes
    d = OnDevice(blank())
    dxyz = d.upload(np.asarray(xyz, np.float64))
    doff, dimg = d.upload(np.asarray(off, np.int32)), d.upload(np.asarray(img, np.int32))
    sph = np.array(sphere, np.float64)
    d.call(L.hpmvs_init_patches_sphere_batch, gpu_scene.h, C.byref(o), 2, n, dxyz.data_ptr(), doff.data_ptr(), dimg.data_ptr(),
           sph.ctypes.data, C.byref(d.pb))
    for k in api.Batch.FIELDS:
        assert same_bytes(d.t[k].cpu().numpy(), getattr(want, k)), k

    # sphere == NULL is hpmvs_init_patches_batch; r = +inf gates nothing
    def host_call(sphere_ptr):
        b = blank()
        pb = b.c_struct()
        rc = L.hpmvs_init_patches_sphere_batch(gpu_scene.h, C.byref(o), 2, n, xyz.ctypes.data, off.ctypes.data, img.ctypes.data,
                                               sphere_ptr, C.byref(pb), 0, None)
        return rc, b

    xyz, off, img = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(off, np.int32), np.ascontiguousarray(img, np.int32)
    rc, b = host_call(None)
    assert rc == 0
    for k in api.Batch.FIELDS:
        assert same_bytes(getattr(b, k), getattr(plain, k)), k
    everything = api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, sphere=(0.0, 0.0, 0.0, np.inf))
    for k in api.Batch.FIELDS:
        assert same_bytes(getattr(everything, k), getattr(plain, k)), k

    # no sphere at all: HPMVS_ERR_ARG
    for bad in ((np.nan, 0.0, 0.0, 5.0), (0.0, np.inf, 0.0, 5.0), (0.0, 0.0, 0.0, -1.0), (0.0, 0.0, 0.0, np.nan)):
        s = np.array(bad, np.float64)
        rc, _ = host_call(s.ctypes.data)
        assert rc == ERR_ARG, bad
        with pytest.raises(api.HpmvsError, match="error -2"):
            api.init_patches_batch(gpu_scene, xyz, off, img, start_level=2, sphere=bad)
    rc, b = host_call(np.array((0.0, 0.0, 0.0, 0.0), np.float64).ctypes.data)  # r = 0 is a sphere
    assert rc == 0 and (b.stage == 13).all()
