"""hpmvs_scene_center (Scene::getSceneCenter of the reference, host code, no GPU) against tests/scene_center_ref.py.

The tolerance is not tuned: two backward-stable solutions of the same 4x4 system agree to
64 * 2^-52 * |A^-1|_2 (|A|_2 |x|_2 + |b|_2), computed per camera set from the restatement's own A and b and applied to the centre
(2-norm) and to the radius, which is a distance from that centre.  For the configs[0] cameras it is 4.3e-13 (centre ~ 0, radius
30, cond(A) = 15.3; the float32 camera tables move that centre by about 2e-6, which both sides see alike)."""
import ctypes as C

import numpy as np
import pytest

import scene_center_ref as ref


def _tables(cams):
    return np.array([list(c.zaxis) for c in cams], np.float32), np.array([list(c.center) for c in cams], np.float32)


def _from_views(views):
    from hpmvs_amd import api
    return [api.camera_from_nvm(v.f, v.q, v.c, v.width, v.height) for v in views]


def _random_views(n, seed):
    """centres in [-10, 10]^3, rotations from random unit quaternions: optical axes that do not meet"""
    from hpmvs_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    views = []
    for _ in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        views.append(synth.View(640, 480, 768.0, q, rng.uniform(-10.0, 10.0, size=3)))
    return views


def _camera_sets():
    from hpmvs_amd import synth
    return {
        "configs0": synth.make_cameras(3, 640, 480),
        "random8": _random_views(8, 20260),
        "two": _random_views(2, 20261),
        "ring200": synth.make_cameras(200, 640, 480),
    }


@pytest.mark.parametrize("name", ["configs0", "random8", "two", "ring200"])
def test_scene_center_matches_restatement(name):
    from hpmvs_amd import api
    cams = _from_views(_camera_sets()[name])
    zaxis, center = _tables(cams)
    want = ref.scene_center(zaxis, center)
    assert want is not None
    bound = ref.solve_bound(zaxis, center)
    got = api.scene_center(cams)
    assert got is not None
    dc, dr = float(np.linalg.norm(got[0] - want[0])), abs(got[1] - want[1])
    print(f"{name}: centre {got[0]} radius {got[1]!r} |d centre| {dc:.3e} |d radius| {dr:.3e} bound {bound:.3e}")
    assert got[0].dtype == np.float64 and got[1] > 0.0
    assert dc <= bound and dr <= bound
    if name == "configs0":
        # the ring looks at the origin from 30 away; the tables are float32 (30 * 2^-24 = 1.8e-6 per coordinate, cond(A) = 15.3)
        assert bound < 1e-12 and np.linalg.norm(got[0]) < 1e-4 and abs(got[1] - 30.0) < 1e-4


def test_radius_is_the_largest_distance_not_the_median():
    from hpmvs_amd import api
    cams = _from_views(_random_views(8, 20260))
    c, r = api.scene_center(cams)
    _, center = _tables(cams)
    d = np.sort(np.linalg.norm(center[:, :3].astype(np.float64) - c, axis=1))
    assert abs(r - d[-1]) <= 4 * ref.EPS * d[-1] and r > d[len(d) // 2]


def test_no_valid_centre():
    from hpmvs_amd import api
    cams = _from_views(_random_views(4, 20262))
    assert api.scene_center([]) is None          # the reference returns false
    assert api.scene_center(cams[:1]) is None    # the reference aborts on its CHECK; here: no centre
    for axis in ((0.0, 0.0, 1.0), (1.0, 2.0, 3.0)):
        same = []
        for c in cams:  # four centres, one optical axis: the 3x3 block has rank 2
            k = api.Camera.from_buffer_copy(c)
            z = np.asarray(axis, np.float32) / np.float32(np.linalg.norm(np.asarray(axis, np.float32)))
            k.zaxis[0], k.zaxis[1], k.zaxis[2] = (float(t) for t in z)
            same.append(k)
        assert api.scene_center(same) is None and ref.scene_center(*_tables(same)) is None
    assert api.scene_center(cams) is not None


def test_bad_arguments():
    from hpmvs_amd import api
    L = api.lib()
    cams = (api.Camera * 2)(*_from_views(_random_views(2, 20261)))
    center, radius, valid = (C.c_double * 3)(), C.c_double(), C.c_int()
    ERR_ARG = -2
    assert L.hpmvs_scene_center(cams, 2, None, C.byref(radius), C.byref(valid)) == ERR_ARG
    assert L.hpmvs_scene_center(cams, 2, center, None, C.byref(valid)) == ERR_ARG
    assert L.hpmvs_scene_center(cams, 2, center, C.byref(radius), None) == ERR_ARG
    assert L.hpmvs_scene_center(None, 2, center, C.byref(radius), C.byref(valid)) == ERR_ARG
    assert L.hpmvs_scene_center(cams, -1, center, C.byref(radius), C.byref(valid)) == ERR_ARG
    assert b"scene_center" in L.hpmvs_last_error()
    assert L.hpmvs_scene_center(None, 0, center, C.byref(radius), C.byref(valid)) == 0 and valid.value == 0
    assert L.hpmvs_scene_center(cams, 2, center, C.byref(radius), C.byref(valid)) == 0 and valid.value == 1
