"""numpy float64 restatement of the reference's --only_sphere (options.FILTER_SCENE_CENTER): the yardstick for
hpmvs_scene_center and for the gate of hpmvs_init_patches_sphere_batch.  It shares nothing with the product's code.

  scene_center  Scene::getSceneCenter, src/hpmvs/Scene.cpp:210-239, over TriangulateMidpoint,
                include/hpmvs/Triangulation.hpp:28-53
  gate          the test in front of the seed loop, src/hpmvs/Scene.cpp:118-121

The reference solves its 4x4 system with Eigen's column-pivoted Householder QR; here it is numpy's LU with partial pivoting.
Both are backward stable, so two solutions of the same system differ by at most `solve_bound`; nothing tighter is claimed.
"""
import numpy as np

EPS = 2.0 ** -52


def _norm3(v):
    """|v| of a 3-vector summed left to right, the order the project's parity contract fixes for such norms."""
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def system(zaxis, center):
    """A (4x4), b (4) and the origins o_i of TriangulateMidpoint (Triangulation.hpp:35-45), accumulated in camera order.
    zaxis [n][3], center [n][4]: the float32 tables of the cameras (Camera::oAxis_.head(3), Camera::center_)."""
    zaxis = np.asarray(zaxis, dtype=np.float64).reshape(-1, 3)
    center = np.asarray(center, dtype=np.float64).reshape(-1, 4)
    A, b = np.zeros((4, 4)), np.zeros(4)
    origins = []
    for z, c in zip(zaxis, center):
        d = z / _norm3(z)                       # rays: oAxis_.head<3>().cast<double>().normalized()   (Scene.cpp:215)
        o = c[:3] / c[3]                        # origins: center_.cast<double>().hnormalized()         (Scene.cpp:216)
        dh = np.array([d[0], d[1], d[2], 0.0])
        oh = np.array([o[0], o[1], o[2], 1.0])
        A_term = np.eye(4) - np.outer(dh, dh)   # Triangulation.hpp:41-42
        A += A_term                             # :43
        Ao = np.array([((A_term[r, 0] * oh[0] + A_term[r, 1] * oh[1]) + A_term[r, 2] * oh[2]) + A_term[r, 3] * oh[3]
                       for r in range(4)])
        b += Ao                                 # :44
        origins.append(o)
    return A, b, np.array(origins).reshape(-1, 3)


def scene_center(zaxis, center):
    """(center[3], radius), or None where Scene::getSceneCenter has no answer: no camera (Scene.cpp:218-219), one camera
    (CHECK_GE(origins.size(), 2), Triangulation.hpp:32) or a singular system."""
    A, b, origins = system(zaxis, center)
    if len(origins) < 2 or np.linalg.matrix_rank(A) < 4:
        return None
    x = np.linalg.solve(A, b)                   # Triangulation.hpp:47-51
    c = x[:3] / x[3]                            # center_homog.hnormalized()   (Scene.cpp:225)
    radius = max(_norm3(c - o) for o in origins)   # dists[dists.size() - 1] of the sorted distances: the maximum  (:233)
    return c, float(radius)


def solve_bound(zaxis, center):
    """64 * 2^-52 * |A^-1| (|A| |x| + |b|) in 2-norms: how far two backward-stable solutions of A x = b can lie apart."""
    A, b, _ = system(zaxis, center)
    x = np.linalg.solve(A, b)
    return 64.0 * EPS * np.linalg.norm(np.linalg.inv(A), 2) * (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))


def gate(xyz, sphere):
    """bool [n]: the points Scene.cpp:119 skips, (pt.xyz - sceneCenter).norm() > sceneRadius, in float64.  A NaN distance
    compares false (kept), an infinite one true unless the radius is infinite as well."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    cx, cy, cz, r = (np.float64(t) for t in sphere)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = xyz[:, 0] - cx, xyz[:, 1] - cy, xyz[:, 2] - cz
        dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
        return dist > r
