"""ctypes binding of the product C ABI (include/hpmvs_amd.h -> hpmvs_amd/libhpmvs_amd.so).

Plumbing only: it loads the in-tree shared library (built by `__graft_entry__.build()` /
`make -C hpmvs_amd/csrc`), marshals numpy arrays or raw device pointers, and raises on any
non-zero status.  There is no Python or CPU implementation of the hot path behind it: if the
library or a GPU is missing the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

try:  # torch first: it must be the one to load libamdhip64 ("one HIP runtime")
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional plumbing
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPMVS_LIB") or os.path.join(HERE, "libhpmvs_amd.so")   # (HPMVS_LIB: a variant build, measurements only)
MAX_IMAGES = 256   # HPMVS_MAX_IMAGES: ids per list row the C ABI takes
FAST_IMAGES = 64   # HPMVS_FAST_IMAGES: lists that never outgrow this run in the batch kernel alone
MAX_LEVELS = 8


class HpmvsError(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [("MAXLEVEL", C.c_int32), ("MINLEVEL", C.c_int32), ("MAX_ANGLE", C.c_float),
                ("MIN_ANGLE", C.c_float), ("MAX_IMAGES_PER_PATCH", C.c_int32),
                ("MIN_IMAGES_PER_PATCH", C.c_int32), ("NCC_ALPHA_1", C.c_float), ("NCC_ALPHA_2", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("P0", C.c_float * 12), ("center", C.c_float * 4), ("xaxis", C.c_float * 3),
                ("yaxis", C.c_float * 3), ("zaxis", C.c_float * 3), ("fsum", C.c_float), ("n_levels", C.c_int32)]


class PatchBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("max_images", C.c_int32), ("center", C.c_void_p), ("normal", C.c_void_p),
                ("scale", C.c_void_p), ("n_images", C.c_void_p), ("images", C.c_void_p), ("ok", C.c_void_p),
                ("color", C.c_void_p), ("ncc", C.c_void_p), ("fmin", C.c_void_p), ("x", C.c_void_p),
                ("result", C.c_void_p), ("nevals", C.c_void_p), ("stage", C.c_void_p), ("ngrabs", C.c_void_p)]


class LeafTable(C.Structure):
    _fields_ = [("n", C.c_int32), ("root_center", C.c_float * 3), ("root_width", C.c_float), ("cell_center", C.c_void_p),
                ("cell_width", C.c_void_p), ("patch_center", C.c_void_p), ("born", C.c_void_p), ("died", C.c_void_p)]


class OctreeIndex(C.Structure):
    _fields_ = [("root_center", C.c_float * 3), ("root_width", C.c_float), ("n_branches", C.c_int32), ("n_leaves", C.c_int32),
                ("branch_key", C.c_void_p), ("leaf_key", C.c_void_p)]


class ExtendTreeKeysStruct(C.Structure):
    _fields_ = [("skip", C.c_void_p), ("pre_inside", C.c_void_p), ("pre_key", C.c_void_p), ("border", C.c_void_p),
                ("post_key", C.c_void_p)]


class OctreeForest(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("root", C.c_void_p), ("branch_first", C.c_void_p), ("leaf_first", C.c_void_p),
                ("branch_key", C.c_void_p), ("leaf_key", C.c_void_p)]


class ProcessForestResultStruct(C.Structure):
    _fields_ = [("support", C.c_void_p), ("removed", C.c_void_p), ("split", C.c_void_p), ("children", C.c_void_p),
                ("child_key", C.c_void_p), ("n_neighbours", C.c_void_p), ("neighbour_key", C.c_void_p)]


class BorderForestResultStruct(C.Structure):
    _fields_ = [("tree", C.c_void_p), ("accepted", C.c_void_p), ("leaf_key", C.c_void_p), ("blocker", C.c_void_p)]


class OctreePartitionInfo(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("n_orphans", C.c_int32), ("n_splits", C.c_int32), ("stop", C.c_int32),
                ("histogram", C.c_int32 * 22)]


class SeedTreeInfo(C.Structure):
    _fields_ = [("root_center", C.c_float * 3), ("root_width", C.c_float), ("scale_floor", C.c_float), ("n_rows", C.c_int32),
                ("n_leaves", C.c_int32)]


EXPORTS = [
    "hpmvs_last_error", "hpmvs_device_count", "hpmvs_build_id", "hpmvs_default_options", "hpmvs_camera_from_nvm",
    "hpmvs_scene_create", "hpmvs_scene_set_view", "hpmvs_scene_set_covis", "hpmvs_scene_commit",
    "hpmvs_scene_destroy", "hpmvs_scene_get_level", "hpmvs_scene_bytes", "hpmvs_build_pyramid",
    "hpmvs_optimize_batch", "hpmvs_init_patches_batch", "hpmvs_objective_batch", "hpmvs_inccs_batch", "hpmvs_last_kernel_ms",
    "hpmvs_last_wide_patches",
    "hpmvs_expand_batch", "hpmvs_expand_directions", "hpmvs_selftest_bobyqa",
    "hpmvs_pack_records", "hpmvs_unpack_records", "hpmvs_allgather_records", "hpmvs_pack_record_tails", "hpmvs_unpack_record_tails",
    "hpmvs_scene_depth_reset", "hpmvs_scene_depth_set_level", "hpmvs_scene_depth_get_level",
    "hpmvs_set_depths_batch", "hpmvs_depth_gates_batch", "hpmvs_depth_footprints_batch", "hpmvs_depth_ops_batch", "hpmvs_level_support_batch",
    "hpmvs_host_alloc", "hpmvs_host_free", "hpmvs_last_staging",
    "hpmvs_undistort", "hpmvs_undistort_map", "hpmvs_scene_set_view_distorted",
    "hpmvs_regularize_batch", "hpmvs_filter_batch", "hpmvs_seed_tree_batch", "hpmvs_octree_locate_batch",
    "hpmvs_octree_insert_batch", "hpmvs_octree_route_batch", "hpmvs_octree_partition", "hpmvs_extend_tree_batch",
    "hpmvs_extend_forest_batch", "hpmvs_process_forest_batch", "hpmvs_border_forest_batch",
    "hpmvs_level_conflicts_batch", "hpmvs_conflicts_from_footprints", "hpmvs_level_walk_batch", "hpmvs_last_level_walk",
    "hpmvs_scene_center", "hpmvs_init_patches_sphere_batch",
    "hpmvs_jpeg_info", "hpmvs_jpeg_decode", "hpmvs_scene_set_view_jpeg", "hpmvs_jpeg_decode_timed",
    "hpmvs_jpeg_decode_ex", "hpmvs_scene_set_view_jpeg_ex", "hpmvs_jpeg_coefficients", "hpmvs_jpeg_entropy_timed",
    "hpmvs_jpeg_last_decode",
    "hpmvs_jpeg_encode_bound", "hpmvs_jpeg_encode", "hpmvs_jpeg_encode_timed", "hpmvs_scene_get_level_jpeg",
    "hpmvs_depth_colormap", "hpmvs_scene_depth_image", "hpmvs_scene_depth_jpeg",
    "hpmvs_ply_ext_batch", "hpmvs_ply_ext_timed",
]
JPEG_ENTROPY = {"auto": 0, "host": 1, "device": 2}   # HPMVS_JPEG_ENTROPY_AUTO / _HOST / _DEVICE


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HpmvsError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no fallback implementation)")
    L = C.CDLL(LIB_PATH)
    L.hpmvs_last_error.restype = C.c_char_p
    L.hpmvs_build_id.restype = C.c_char_p
    L.hpmvs_default_options.argtypes = [C.POINTER(Options)]
    L.hpmvs_camera_from_nvm.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                        C.c_int, C.POINTER(Camera)]
    L.hpmvs_scene_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.hpmvs_scene_set_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(Camera)]
    L.hpmvs_scene_set_covis.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.hpmvs_scene_commit.argtypes = [C.c_void_p]
    L.hpmvs_scene_destroy.argtypes = [C.c_void_p]
    L.hpmvs_scene_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    L.hpmvs_scene_bytes.restype = C.c_size_t
    L.hpmvs_scene_bytes.argtypes = [C.c_void_p]
    L.hpmvs_build_pyramid.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.hpmvs_undistort.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int]
    L.hpmvs_undistort_map.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.hpmvs_scene_set_view_distorted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.POINTER(Camera), C.c_float, C.c_float]
    L.hpmvs_jpeg_info.argtypes = [C.c_char_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5
    L.hpmvs_jpeg_decode.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    L.hpmvs_jpeg_decode_timed.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_float)]
    L.hpmvs_scene_set_view_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(Camera), C.c_float, C.c_float]
    L.hpmvs_jpeg_decode_ex.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.hpmvs_scene_set_view_jpeg_ex.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(Camera), C.c_float, C.c_float,
                                               C.c_int, C.POINTER(C.c_int)]
    L.hpmvs_jpeg_coefficients.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hpmvs_jpeg_last_decode.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hpmvs_jpeg_entropy_timed.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_float)]
    L.hpmvs_jpeg_encode_bound.restype = C.c_size_t
    L.hpmvs_jpeg_encode_bound.argtypes = [C.c_int, C.c_int]
    L.hpmvs_jpeg_encode.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.hpmvs_jpeg_encode_timed.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_float)]
    L.hpmvs_scene_get_level_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hpmvs_optimize_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(PatchBatch), C.c_int, C.c_void_p]
    L.hpmvs_init_patches_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_void_p]
    L.hpmvs_init_patches_sphere_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_void_p]
    L.hpmvs_scene_center.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.hpmvs_objective_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(PatchBatch), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_inccs_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(PatchBatch), C.c_int, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.hpmvs_host_alloc.argtypes = [C.c_size_t]
    L.hpmvs_host_alloc.restype = C.c_void_p
    L.hpmvs_host_free.argtypes = [C.c_void_p]
    L.hpmvs_host_free.restype = None
    L.hpmvs_last_staging.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.hpmvs_expand_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.c_int, C.POINTER(PatchBatch), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_void_p]
    L.hpmvs_expand_directions.argtypes = [C.c_int, C.c_void_p]
    L.hpmvs_scene_depth_reset.argtypes = [C.c_void_p]
    L.hpmvs_scene_depth_set_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.hpmvs_scene_depth_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]
    L.hpmvs_depth_colormap.argtypes = [C.c_void_p]
    L.hpmvs_scene_depth_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.hpmvs_scene_depth_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hpmvs_set_depths_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_void_p]
    L.hpmvs_depth_footprints_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]
    L.hpmvs_level_conflicts_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                              C.c_int, C.c_void_p]
    L.hpmvs_conflicts_from_footprints.argtypes = [C.c_int] * 5 + [C.c_void_p] * 6 + [C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                  C.c_int, C.c_void_p]
    L.hpmvs_level_walk_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(PatchBatch)] + [C.c_void_p] * 4 + [C.c_float, C.c_int] + \
        [C.c_void_p] * 4 + [C.POINTER(C.c_int32), C.c_int, C.c_void_p]
    L.hpmvs_last_level_walk.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 3
    L.hpmvs_depth_gates_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_depth_ops_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_regularize_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LeafTable),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_level_support_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_filter_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_seed_tree_batch.argtypes = [C.c_void_p, C.POINTER(PatchBatch), C.c_int, C.c_int, C.POINTER(SeedTreeInfo), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_octree_locate_batch.argtypes = [C.c_void_p, C.POINTER(OctreeIndex), C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]
    L.hpmvs_octree_insert_batch.argtypes = [C.c_void_p, C.POINTER(OctreeIndex), C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    L.hpmvs_extend_tree_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(OctreeIndex), C.POINTER(PatchBatch), C.c_float,
                                          C.POINTER(PatchBatch), C.POINTER(ExtendTreeKeysStruct), C.c_int, C.c_void_p]
    L.hpmvs_extend_forest_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(OctreeForest), C.POINTER(PatchBatch), C.c_void_p,
                                            C.c_float, C.POINTER(PatchBatch), C.POINTER(ExtendTreeKeysStruct), C.c_int, C.c_void_p]
    L.hpmvs_process_forest_batch.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(OctreeForest), C.c_void_p, C.POINTER(PatchBatch),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PatchBatch),
                                             C.POINTER(ProcessForestResultStruct), C.c_int, C.c_void_p]
    L.hpmvs_border_forest_batch.argtypes = [C.c_void_p, C.POINTER(OctreeForest), C.POINTER(PatchBatch), C.c_int,
                                            C.POINTER(BorderForestResultStruct), C.c_int, C.c_void_p]
    L.hpmvs_octree_route_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.hpmvs_octree_partition.argtypes = [C.c_void_p, C.POINTER(OctreeIndex), C.c_int, C.c_int, C.POINTER(OctreePartitionInfo)] + \
        [C.c_void_p] * 9 + [C.c_int, C.c_void_p]
    L.hpmvs_ply_ext_batch.argtypes = [C.c_int, C.POINTER(PatchBatch), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.c_int, C.c_void_p]
    L.hpmvs_ply_ext_timed.argtypes = [C.c_int, C.POINTER(PatchBatch), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_float)]
    _lib = L
    return L


def _chk(rc):
    if rc != 0:
        raise HpmvsError(f"hpmvs_amd error {rc}: {lib().hpmvs_last_error().decode()}")


def build_id() -> str:
    """Source hash the loaded library was built from (stamped by hpmvs_amd/csrc/Makefile)."""
    return lib().hpmvs_build_id().decode()


def device_count() -> int:
    return lib().hpmvs_device_count()


def default_options() -> Options:
    o = Options()
    lib().hpmvs_default_options(C.byref(o))
    return o


def camera_from_nvm(f, q, c, width, height, max_level=5) -> Camera:
    cam = Camera()
    qq = (C.c_double * 4)(*[float(t) for t in q])
    cc = (C.c_double * 3)(*[float(t) for t in c])
    _chk(lib().hpmvs_camera_from_nvm(float(f), qq, cc, int(width), int(height), int(max_level), C.byref(cam)))
    return cam


def scene_center(cameras):
    """Scene::getSceneCenter (reference Scene.cpp:210-239) for a sequence of Camera structs, e.g. Scene.cameras: the point
    closest to every optical axis and the largest distance from it to a camera centre, as (center[3] float64, radius), or None
    where the reference has no valid centre (fewer than 2 cameras, parallel axes).  Host code; needs no GPU."""
    cams = (Camera * max(1, len(cameras)))(*cameras)
    center, radius, valid = (C.c_double * 3)(), C.c_double(), C.c_int()
    _chk(lib().hpmvs_scene_center(cams, len(cameras), center, C.byref(radius), C.byref(valid)))
    if not valid.value:
        return None
    return np.array(center[:], dtype=np.float64), radius.value


def _ptr(a):
    """numpy array / torch tensor / int -> raw address (or None)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, int):
        return a
    return a.data_ptr()  # torch tensor


def undistort(img, f: float, k1: float, device: int = 0):
    """Image::undistort of the reference on the GPU: raw level 0 (uint8 [H, W, 3], numpy or a device tensor) -> the
    undistorted level 0 of the same type and place.  Pixels the reference never writes are 0; k1 == 0 returns a copy."""
    if isinstance(img, np.ndarray):
        src = np.ascontiguousarray(img, dtype=np.uint8)
        if src.ndim != 3 or src.shape[2] != 3:
            raise HpmvsError("undistort: img must be uint8 [H, W, 3]")
        out = np.empty_like(src)
        _chk(lib().hpmvs_undistort(device, src.ctypes.data, src.shape[1], src.shape[0], float(f), float(k1),
                                   out.ctypes.data, 0))
        return out
    src = img.contiguous()
    if src.dim() != 3 or src.shape[2] != 3 or str(src.dtype) != "torch.uint8":
        raise HpmvsError("undistort: img must be uint8 [H, W, 3]")
    out = torch.empty_like(src)
    _chk(lib().hpmvs_undistort(device, src.data_ptr(), src.shape[1], src.shape[0], float(f), float(k1), out.data_ptr(), 1))
    return out


def undistort_map(w: int, h: int, f: float, k1: float, device: int = 0) -> np.ndarray:
    """float32 [h, w, 2]: the level-0 point (x, y) each output pixel of hpmvs_undistort samples (NaN included)."""
    xy = np.empty((int(h), int(w), 2), dtype=np.float32)
    _chk(lib().hpmvs_undistort_map(device, int(w), int(h), float(f), float(k1), xy.ctypes.data))
    return xy


def jpeg_info(data):
    """(width, height, components, h_samp, v_samp) of a JPEG file held in a bytes-like object.  Host code; needs no GPU.  Raises
    for a file hpmvs_jpeg_decode would refuse (HPMVS_ERR_UNSUPPORTED = -5, or -2 for a malformed or truncated one)."""
    data = bytes(data)
    v = [C.c_int() for _ in range(5)]
    _chk(lib().hpmvs_jpeg_info(data, len(data), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _jpeg_entropy(name):
    if name not in JPEG_ENTROPY:
        raise HpmvsError(f"entropy must be one of {sorted(JPEG_ENTROPY)}, not {name!r}")
    return JPEG_ENTROPY[name]


def jpeg_decode(data, device: int = 0, on_device: bool = False, entropy: str = "auto"):
    """Baseline JPEG file (bytes-like) -> uint8 [H, W, 3] with libjpeg's default pixels, everything behind the entropy decode on
    the GPU.  A numpy array, or with on_device a torch tensor on the device (the pixels never visit the host).
    entropy: where the Huffman scan is decoded -- "auto" (the library's choice, or what HPMVS_JPEG_ENTROPY names), "host", or
    "device" (the GPU itself: a scan it does not take raises HPMVS_ERR_STATE = -3 instead of falling back).  The pixels do not
    depend on it."""
    data = bytes(data)
    mode = _jpeg_entropy(entropy)
    w, h = jpeg_info(data)[:2]
    if on_device:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=f"cuda:{device}")
        ptr, nb = out.data_ptr(), out.numel()
    else:
        out = np.empty((h, w, 3), dtype=np.uint8)
        ptr, nb = out.ctypes.data, out.nbytes
    if mode == 0:
        _chk(lib().hpmvs_jpeg_decode(device, data, len(data), ptr, nb, int(on_device)))
    else:
        _chk(lib().hpmvs_jpeg_decode_ex(device, data, len(data), ptr, nb, int(on_device), mode, None))
    return out


def jpeg_coefficients(data, entropy: str = "auto", subseq_bits: int = 0, device: int = 0):
    """The dense coefficients behind the entropy decode -> (int16 array: per component [blocks_y][blocks_x][64], one component behind
    the other; "host" or "device", what decoded the scan; synchronisation rounds of the device decode).  subseq_bits: the device
    decode's subsequence size, 0 for the shipped one, else a multiple of 32 from 64 up (a test hook)."""
    data = bytes(data)
    w, h, comps, hs, vs = jpeg_info(data)
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    out = np.empty(64 * mx * my * (hs * vs + (2 if comps == 3 else 0)), dtype=np.int16)
    used, rounds = C.c_int(), C.c_int()
    _chk(lib().hpmvs_jpeg_coefficients(device, data, len(data), _jpeg_entropy(entropy), int(subseq_bits), out.ctypes.data, out.size,
                                       C.byref(used), C.byref(rounds)))
    return out, "device" if used.value == 2 else "host", rounds.value


def jpeg_encode_bound(width: int, height: int) -> int:
    """Upper bound in bytes of jpeg_encode's file for a width x height image, at any quality."""
    return int(lib().hpmvs_jpeg_encode_bound(int(width), int(height)))


def jpeg_encode(rgb, quality: int = 100, device: int = 0) -> bytes:
    """uint8 [H, W, 3] pixels (a numpy array, or a torch tensor on the device, which is read in place) -> the baseline JPEG file
    libjpeg writes for them with its defaults at `quality` (YCbCr 4:2:0, the standard Huffman tables), byte for byte; colour
    conversion, DCT, Huffman coding and byte stuffing run on the GPU.  Raises for a quality outside 1 .. 100 or a side above
    65535 (HPMVS_ERR_ARG = -2) and for a side under 8 pixels (HPMVS_ERR_UNSUPPORTED = -5)."""
    if isinstance(rgb, np.ndarray):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        ptr, on_device = rgb.ctypes.data, 0
    else:
        rgb = rgb.contiguous()
        ptr, on_device = rgb.data_ptr(), 1
    if rgb.ndim != 3 or rgb.shape[2] != 3 or (on_device and rgb.dtype != torch.uint8):
        raise HpmvsError("jpeg_encode: pixels must be uint8 [H, W, 3]")
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    out = np.empty(max(1, jpeg_encode_bound(w, h)), dtype=np.uint8)
    n = C.c_size_t(0)
    _chk(lib().hpmvs_jpeg_encode(device, ptr, w, h, int(quality), out.ctypes.data, out.nbytes, C.byref(n), on_device))
    return out[:n.value].tobytes()


class Scene:
    """HBM-resident scene: Scene::addCameras + extractCoVisiblilty state the path reads
    (reference include/hpmvs/Scene.h:69-71)."""

    def __init__(self, synth_scene, device: int = 0, jpeg_entropy: str = "auto"):
        L = lib()
        jpeg_mode = _jpeg_entropy(jpeg_entropy)   # where views given as JPEG bytes have their scans decoded (jpeg_decode)
        self.h = C.c_void_p()
        self.device = device
        self.n_views = synth_scene.n_views
        self.view_levels = []   # pyramid levels per view (Camera::getLevels)
        self.cameras = []       # the hpmvs_camera structs of the views (scene_center(scene.cameras))
        _chk(L.hpmvs_scene_create(self.n_views, device, C.byref(self.h)))
        for i, v in enumerate(synth_scene.views):
            rgb = v.rgb
            if isinstance(rgb, (bytes, bytearray)):  # a JPEG file as VisualSFM names it: decoded (and undistorted) in HBM
                data = bytes(rgb)
                w, h = jpeg_info(data)[:2]
                cam = camera_from_nvm(v.f, v.q, v.c, w, h, synth_scene.max_level)
                self.view_levels.append(int(cam.n_levels))
                self.cameras.append(cam)
                if jpeg_mode == 0:
                    _chk(L.hpmvs_scene_set_view_jpeg(self.h, i, data, len(data), C.byref(cam), float(v.f),
                                                     float(getattr(v, "k1", 0.0))))
                else:
                    _chk(L.hpmvs_scene_set_view_jpeg_ex(self.h, i, data, len(data), C.byref(cam), float(v.f),
                                                        float(getattr(v, "k1", 0.0)), jpeg_mode, None))
                continue
            cam = camera_from_nvm(v.f, v.q, v.c, v.width, v.height, synth_scene.max_level)
            self.view_levels.append(int(cam.n_levels))
            self.cameras.append(cam)
            if isinstance(rgb, np.ndarray):
                rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
                ptr, on_device = rgb.ctypes.data, 0
            else:  # torch tensor already in HBM
                rgb = rgb.contiguous()
                ptr, on_device = rgb.data_ptr(), 1
            k1 = float(getattr(v, "k1", 0.0))
            if k1 != 0.0:  # raw pixels of a camera with radial distortion: undistorted on the GPU (Image::load)
                _chk(L.hpmvs_scene_set_view_distorted(self.h, i, v.width, v.height, ptr, on_device, C.byref(cam),
                                                      float(v.f), k1))
            else:
                _chk(L.hpmvs_scene_set_view(self.h, i, v.width, v.height, ptr, on_device, C.byref(cam)))
        for i, lst in enumerate(synth_scene.covis):
            arr = (C.c_int32 * max(1, len(lst)))(*lst)
            _chk(L.hpmvs_scene_set_covis(self.h, i, arr, len(lst)))
        _chk(L.hpmvs_scene_commit(self.h))

    def close(self):
        if self.h:
            lib().hpmvs_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bytes(self) -> int:
        return lib().hpmvs_scene_bytes(self.h)

    def level(self, view: int, level: int) -> np.ndarray:
        w, h = C.c_int(), C.c_int()
        _chk(lib().hpmvs_scene_get_level(self.h, view, level, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 3), dtype=np.uint8)
        _chk(lib().hpmvs_scene_get_level(self.h, view, level, out.ctypes.data, out.nbytes, C.byref(w), C.byref(h)))
        return out

    def level_jpeg(self, view: int, level: int = 0, quality: int = 100) -> bytes:
        """The level as the baseline JPEG file jpeg_encode writes for its pixels, encoded where it lies in HBM (level 0 of a view
        with k1 != 0: the undistorted pixels)."""
        n = C.c_size_t(0)
        _chk(lib().hpmvs_scene_get_level_jpeg(self.h, view, level, int(quality), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        _chk(lib().hpmvs_scene_get_level_jpeg(self.h, view, level, int(quality), out.ctypes.data, out.nbytes, C.byref(n)))
        return out[:n.value].tobytes()

    def depth_image(self, view: int, level=None, with_range: bool = False):
        """One depth map of the view (level None: the minimum over all levels, Scene::getFullDepth) as the jet-coloured image
        the reference's Scene::visualizeDepths saves: uint8 [rows, cols, 3], rendered from the maps where they lie in HBM.
        with_range: -> (image, (m, M)), the least and largest value the normalisation used."""
        lv = DEPTH_COMBINED if level is None else int(level)
        w, h = C.c_int(), C.c_int()
        _chk(lib().hpmvs_scene_depth_image(self.h, view, lv, None, 0, 0, C.byref(w), C.byref(h), None))
        out = np.empty((h.value, w.value, 3), dtype=np.uint8)
        rng = (C.c_float * 2)()
        _chk(lib().hpmvs_scene_depth_image(self.h, view, lv, out.ctypes.data if out.size else None, out.nbytes, 0, C.byref(w), C.byref(h), rng))
        return (out, (np.float32(rng[0]), np.float32(rng[1]))) if with_range else out

    def depth_jpeg(self, view: int, level=None, quality: int = 100) -> bytes:
        """depth_image as the baseline JPEG file jpeg_encode writes for it; neither the cells nor the pixels visit the host.
        Raises for a map under 8 cells on a side (HPMVS_ERR_UNSUPPORTED = -5)."""
        lv = DEPTH_COMBINED if level is None else int(level)
        n = C.c_size_t(0)
        _chk(lib().hpmvs_scene_depth_jpeg(self.h, view, lv, int(quality), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        _chk(lib().hpmvs_scene_depth_jpeg(self.h, view, lv, int(quality), out.ctypes.data, out.nbytes, C.byref(n)))
        return out[:n.value].tobytes()

    def last_staging(self):
        """(bytes copied through device buffers, bytes used in place) of the last host-pointer optimize_batch call."""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        _chk(lib().hpmvs_last_staging(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_wide_patches(self) -> int:
        """Patches of the last refinement launch whose list outgrew 64 ids and that the wide kernel redid."""
        n = C.c_int32()
        _chk(lib().hpmvs_last_wide_patches(self.h, C.byref(n)))
        return n.value

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().hpmvs_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


class Batch:
    """Host-side (numpy) structure-of-arrays Patch3d batch."""

    def __init__(self, center, normal, scale, n_images, images):
        self.n = int(len(scale))
        self.max_images = int(images.shape[1])
        self.center = np.ascontiguousarray(center, dtype=np.float32).copy()
        self.normal = np.ascontiguousarray(normal, dtype=np.float32).copy()
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).copy()
        self.n_images = np.ascontiguousarray(n_images, dtype=np.int32).copy()
        self.images = np.ascontiguousarray(images, dtype=np.int32).copy()
        n = self.n
        self.ok = np.zeros(n, dtype=np.uint8)
        self.color = np.zeros((n, 3), dtype=np.float32)
        self.ncc = np.zeros(n, dtype=np.float32)
        self.fmin = np.zeros(n, dtype=np.float64)
        self.x = np.zeros((n, 3), dtype=np.float64)
        self.result = np.zeros(n, dtype=np.int32)
        self.nevals = np.zeros(n, dtype=np.int32)
        self.stage = np.zeros(n, dtype=np.int32)
        self.ngrabs = np.zeros(n, dtype=np.int32)

    @classmethod
    def from_seeds(cls, seeds, idx=None):
        if idx is None:
            idx = np.arange(len(seeds.scale))
        idx = np.asarray(idx)
        return cls(seeds.center[idx], seeds.normal[idx], seeds.scale[idx], seeds.n_images[idx], seeds.images[idx])

    FIELDS = ("center", "normal", "scale", "n_images", "images", "ok", "color", "ncc", "fmin", "x", "result", "nevals",
              "stage", "ngrabs")

    def pin(self):
        """Move every array into pinned host memory (hpmvs_host_alloc).  Host-pointer calls then use the arrays in place
        (include/hpmvs_amd.h, "Host-pointer calls and pinned memory").  A pinned block lives exactly as long as the last
        numpy view of it: `c = batch.center` stays valid after the Batch is gone, and pinning again releases the previous
        blocks as soon as nothing refers to them."""
        import weakref
        L = lib()
        for name in self.FIELDS:
            a = getattr(self, name)
            nbytes = max(int(a.nbytes), 1)
            p = L.hpmvs_host_alloc(nbytes)
            if not p:
                raise MemoryError(f"hpmvs_host_alloc({nbytes})")
            buf = (C.c_char * nbytes).from_address(p)   # every view of the new array keeps `buf` alive through .base
            weakref.finalize(buf, L.hpmvs_host_free, p)
            na = np.frombuffer(buf, dtype=a.dtype, count=a.size).reshape(a.shape)
            na[...] = a
            setattr(self, name, na)
        return self

    def c_struct(self) -> PatchBatch:
        b = PatchBatch()
        b.n, b.max_images = self.n, self.max_images
        for name in ("center", "normal", "scale", "n_images", "images", "ok", "color", "ncc", "fmin", "x", "result",
                     "nevals", "stage", "ngrabs"):
            setattr(b, name, _ptr(getattr(self, name)))
        return b


def optimize_batch(scene: Scene, batch: Batch, options: Options | None = None) -> Batch:
    o = options or default_options()
    b = batch.c_struct()
    _chk(lib().hpmvs_optimize_batch(scene.h, C.byref(o), C.byref(b), 0, None))
    return batch


def init_patches_batch(scene: Scene, xyz, meas_off, meas_img, start_level=4, max_images=FAST_IMAGES,
                       options: Options | None = None, sphere=None) -> Batch:
    """Scene::initPatches seed loop on the GPU (reference Scene.cpp:112-178): seeds built on device, refined,
    drift-gated.  Returns the batch (seed patches, refined where ok).  max_images: the rows of the batch's image lists; a point
    with more measurements than that ends at stage 100 (the C ABI's maximum, 64, by default: in a 50-view scene most NVM points
    have more than 32).  sphere = (cx, cy, cz, r): the scene-centre gate of --only_sphere (Scene.cpp:118-121), e.g.
    (*center, radius) of scene_center(scene.cameras); a point farther than r from the centre ends at stage 13 before any other
    test.  None: no gate."""
    o = options or default_options()
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    off = np.ascontiguousarray(meas_off, dtype=np.int32)
    img = np.ascontiguousarray(meas_img, dtype=np.int32)
    n = len(xyz)
    batch = Batch(np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32),
                  np.zeros(n, np.int32), np.full((n, max_images), -1, np.int32))
    b = batch.c_struct()
    if sphere is None:
        _chk(lib().hpmvs_init_patches_batch(scene.h, C.byref(o), start_level, n, xyz.ctypes.data, off.ctypes.data,
                                            img.ctypes.data if len(img) else None, C.byref(b), 0, None))
        return batch
    sph = np.ascontiguousarray(sphere, dtype=np.float64).reshape(4)
    _chk(lib().hpmvs_init_patches_sphere_batch(scene.h, C.byref(o), start_level, n, xyz.ctypes.data, off.ctypes.data,
                                               img.ctypes.data if len(img) else None, sph.ctypes.data, C.byref(b), 0, None))
    return batch


EXPAND_EXTEND, EXPAND_BRANCH = 0, 1


def expand_directions(mode: int) -> np.ndarray:
    """(cos, sin) pairs of the candidate directions the expansion kernels use; needs no GPU."""
    out = np.zeros(12, dtype=np.float32)
    n = lib().hpmvs_expand_directions(mode, out.ctypes.data)
    if n < 0:
        _chk(n)
    return out[:2 * n].reshape(n, 2)


def expand_batch(scene: Scene, mode: int, parents: Batch, cell_center, cell_width, skip=None,
                 options: Options | None = None) -> Batch:
    """CellProcessor::extend (mode 0, 6 candidates) / ::branch (mode 1, 4 candidates) for a frontier of parent
    cells (reference CellProcessor.cpp:84-178, 210-262): candidates built, optimized and gated on the GPU.
    Returns the batch of n*N candidates (candidate k of parent i at i*N + k)."""
    o = options or default_options()
    N = 6 if mode == EXPAND_EXTEND else 4
    n = parents.n
    cc = np.ascontiguousarray(cell_center, dtype=np.float32).reshape(n, 3)
    cw = np.ascontiguousarray(cell_width, dtype=np.float32).reshape(n)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(n * N)
    out = Batch(np.zeros((n * N, 4), np.float32), np.zeros((n * N, 4), np.float32), np.zeros(n * N, np.float32),
                np.zeros(n * N, np.int32), np.full((n * N, parents.max_images), -1, np.int32))
    pb, ob = parents.c_struct(), out.c_struct()
    _chk(lib().hpmvs_expand_batch(scene.h, C.byref(o), mode, C.byref(pb), cc.ctypes.data, cw.ctypes.data,
                                  None if sk is None else sk.ctypes.data, C.byref(ob), 0, None))
    return out


def objective_batch(scene: Scene, batch: Batch, x: np.ndarray, options: Options | None = None):
    o = options or default_options()
    b = batch.c_struct()
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = np.zeros(batch.n, dtype=np.float64)
    g = np.zeros(batch.n, dtype=np.int32)
    _chk(lib().hpmvs_objective_batch(scene.h, C.byref(o), C.byref(b), x.ctypes.data, f.ctypes.data, g.ctypes.data, 0,
                                     None))
    return f, g


def inccs_batch(scene: Scene, batch: Batch, ref_idx=0, robust=0, options: Options | None = None) -> np.ndarray:
    o = options or default_options()
    b = batch.c_struct()
    out = np.zeros((batch.n, batch.max_images), dtype=np.float32)
    _chk(lib().hpmvs_inccs_batch(scene.h, C.byref(o), C.byref(b), ref_idx, robust, out.ctypes.data, 0, None))
    return out


def depth_reset(scene: Scene):
    """Allocate (first call) and clear the scene's depth maps (reference Scene.cpp:74-80)."""
    _chk(lib().hpmvs_scene_depth_reset(scene.h))


def depth_level(scene: Scene, view: int, level: int) -> np.ndarray:
    """One depth map in Eigen's storage order: shape (cols, rows), element [x, y]."""
    r, c = C.c_int(), C.c_int()
    _chk(lib().hpmvs_scene_depth_get_level(scene.h, view, level, None, 0, C.byref(r), C.byref(c)))
    out = np.zeros((c.value, r.value), dtype=np.float32)
    _chk(lib().hpmvs_scene_depth_get_level(scene.h, view, level, out.ctypes.data, out.size, C.byref(r), C.byref(c)))
    return out


depth_get_level = depth_level


def depth_set_level(scene: Scene, view: int, level: int, data):
    """One depth map back in, as depth_get_level returned it (shape (cols, rows)): hpmvs_scene_depth_set_level."""
    m = np.ascontiguousarray(data, dtype=np.float32)
    if m.size:   # (a 0-row level: nothing to copy)
        _chk(lib().hpmvs_scene_depth_set_level(scene.h, view, level, m.ctypes.data, m.shape[1], m.shape[0]))


DEPTH_COMBINED = -1   # HPMVS_DEPTH_COMBINED


def depth_colormap() -> np.ndarray:
    """uint8 [256, 3]: the colormap of Scene.depth_image, CImg's jet_LUT256() (host only)."""
    lut = np.zeros((256, 3), dtype=np.uint8)
    _chk(lib().hpmvs_depth_colormap(lut.ctypes.data))
    return lut


def set_depths_batch(scene: Scene, batch: Batch):
    """Scene::setDepths for every patch of the batch with ok != 0 (reference Scene.cpp:351-381)."""
    b = batch.c_struct()
    _chk(lib().hpmvs_set_depths_batch(scene.h, C.byref(b), 0, None))


def depth_ops_batch(scene: Scene, batch: Batch, subtract):
    """Scene::setDepths(patch_i, subtract[i]) for the patches with ok != 0, in batch order, with the sequential loop's maps
    (reference Scene.cpp:351-381; subtract: CellProcessor.cpp:276-279)."""
    b = batch.c_struct()
    sub = np.ascontiguousarray(subtract, dtype=np.uint8).reshape(batch.n)
    _chk(lib().hpmvs_depth_ops_batch(scene.h, C.byref(b), sub.ctypes.data, 0, None))


def level_support_batch(scene: Scene, batch: Batch, min_level=0):
    """Scene::getLevelSupport(patch, min_level) per patch (reference Scene.cpp:334-343)."""
    b = batch.c_struct()
    out = np.zeros(batch.n, dtype=np.int32)
    _chk(lib().hpmvs_level_support_batch(scene.h, C.byref(b), int(min_level), out.ctypes.data, 0, None))
    return out


def depth_gates_batch(scene: Scene, batch: Batch, margin=1.0, abs_int=0):
    """depthTests / viewBlockTest / pixelFreeTests counts per patch (reference Scene.cpp:518-644)."""
    b = batch.c_struct()
    v = np.zeros(batch.n, dtype=np.int32); k = np.zeros(batch.n, dtype=np.int32); f = np.zeros(batch.n, dtype=np.int32)
    _chk(lib().hpmvs_depth_gates_batch(scene.h, C.byref(b), float(margin), int(abs_int), v.ctypes.data, k.ctypes.data,
                                       f.ctypes.data, 0, None))
    return v, k, f


def depth_footprints_batch(scene: Scene, batch: Batch):
    """The depth-map cells the gates of every patch READ and the cells setDepths would WRITE for it (integers; layouts in
    include/hpmvs_amd.h): (writes [n, M, 4], frees [n, M, 4], attached [n, M, 3], view_block [n, n_views, 3])."""
    b = batch.c_struct()
    n, M, V = batch.n, batch.max_images, scene.n_views
    wr = np.zeros((n, M, 4), np.int32); fr = np.zeros((n, M, 4), np.int32)
    at = np.zeros((n, M, 3), np.int32); vb = np.zeros((n, V, 3), np.int32)
    _chk(lib().hpmvs_depth_footprints_batch(scene.h, C.byref(b), wr.ctypes.data, fr.ctypes.data, at.ctypes.data, vb.ctypes.data, 0, None))
    return wr, fr, at, vb


def _conflicts(call, n):
    """The capacity contract of the two conflict-graph calls (include/hpmvs_amd.h): a call with room for 32 edges per node in
    each list; when that does not hold them the totals are valid all the same, and a second call gets arrays of that size.
    call(flow_off, flow_adj, cap_flow, anti_off, anti_adj, cap_anti, n_flow, n_anti) -> status."""
    fo = np.zeros(n + 1, np.uint32); ao = np.zeros(n + 1, np.uint32)
    nf, na = C.c_uint32(0), C.c_uint32(0)
    fa = np.zeros(32 * n + 64, np.uint32); aa = np.zeros(32 * n + 64, np.uint32)
    rc = call(fo.ctypes.data, fa.ctypes.data, fa.size, ao.ctypes.data, aa.ctypes.data, aa.size, C.byref(nf), C.byref(na))
    if rc != 0:
        if "capacity" not in lib().hpmvs_last_error().decode():
            _chk(rc)
        fa = np.zeros(nf.value, np.uint32); aa = np.zeros(na.value, np.uint32)
        _chk(call(fo.ctypes.data, fa.ctypes.data, fa.size, ao.ctypes.data, aa.ctypes.data, aa.size, C.byref(nf), C.byref(na)))
    return fo, fa[:nf.value].copy(), ao, aa[:na.value].copy()


def level_conflicts(scene: Scene, batch: Batch, is_event=None):
    """The conflict graph of one extend level as ONE hpmvs_level_conflicts_batch (include/hpmvs_amd.h): the
    batch's patches are the level's nodes in queue order, is_event marks the subtraction events (None: none).  No footprint
    leaves the device.  Returns (flow_off [n + 1], flow_adj, anti_off [n + 1], anti_adj), uint32, every list ascending."""
    b = batch.c_struct()
    ev = None if is_event is None else np.ascontiguousarray(is_event, dtype=np.uint8).reshape(batch.n)
    evp = None if ev is None else ev.ctypes.data
    return _conflicts(lambda fo, fa, cf, ao, aa, ca, nf, na: lib().hpmvs_level_conflicts_batch(
        scene.h, C.byref(b), evp, fo, fa, cf, ao, aa, ca, nf, na, 0, None), batch.n)


def conflicts_from_footprints(n_images, writes, frees, attached, view_block, n_levels, is_event=None, device: int = 0):
    """The graph step alone, on footprint arrays in the layouts of depth_footprints_batch (writes / frees [n, M, 4], attached
    [n, M, 3], view_block [n, V, 3]; n_images [n]: the entries of a row that count): hpmvs_conflicts_from_footprints.  Needs
    no scene.  Returns what level_conflicts returns."""
    wr = np.ascontiguousarray(writes, dtype=np.int32); fr = np.ascontiguousarray(frees, dtype=np.int32)
    at = np.ascontiguousarray(attached, dtype=np.int32); vb = np.ascontiguousarray(view_block, dtype=np.int32)
    n, M, V = wr.shape[0], wr.shape[1], vb.shape[1]
    if wr.shape != (n, M, 4) or fr.shape != (n, M, 4) or at.shape != (n, M, 3) or vb.shape != (n, V, 3):
        raise ValueError("conflicts_from_footprints: the footprint arrays do not have the layouts of depth_footprints_batch")
    ni = np.ascontiguousarray(n_images, dtype=np.int32).reshape(n)
    ev = None if is_event is None else np.ascontiguousarray(is_event, dtype=np.uint8).reshape(n)
    evp = None if ev is None else ev.ctypes.data
    return _conflicts(lambda fo, fa, cf, ao, aa, ca, nf, na: lib().hpmvs_conflicts_from_footprints(
        int(device), n, M, V, int(n_levels), ni.ctypes.data, wr.ctypes.data, fr.ctypes.data, at.ctypes.data, vb.ctypes.data, evp,
        fo, fa, cf, ao, aa, ca, nf, na, 0, None), n)


WALK_EVENT, WALK_REFINED, WALK_BORDER, WALK_HAS_PRE, WALK_PRE_TAKEN, WALK_POST_TAKEN = 1, 2, 4, 8, 16, 32   # HPMVS_WALK_*


def level_walk(scene: Scene, batch: Batch, flags, set, pre_key, post_key, margin=1.0, abs_int=0, options: Options | None = None,
               stage=None):
    """The wave walk of one extend level as ONE hpmvs_level_walk_batch (include/hpmvs_amd.h): `batch` holds the
    level's queue in the reference's order (an event's patch, a candidate's refined patch), flags the WALK_* bits per item, set
    the tree each candidate's keys belong to (None: one set), pre_key / post_key its leaf before and after refinement.  stage:
    the items' preset stages (default batch.stage).  The scene's depth maps receive the accepted candidates and the events'
    subtractions.  Returns (stage, counts [n, 3], accepted [n] uint8, wave [n] (the 1-based wave that decided the item), n_waves)."""
    o = options or default_options()
    n = batch.n
    b = batch.c_struct()
    fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(n)
    st = None if set is None else np.ascontiguousarray(set, dtype=np.int32).reshape(n)
    pre = np.ascontiguousarray(pre_key, dtype=np.uint64).reshape(n)
    post = np.ascontiguousarray(post_key, dtype=np.uint64).reshape(n)
    stage = np.array(batch.stage if stage is None else stage, dtype=np.int32).reshape(n)
    counts = np.full((n, 3), -1, np.int32); accepted = np.zeros(n, np.uint8); wave = np.zeros(n, np.int32)
    n_waves = C.c_int32(0)
    _chk(lib().hpmvs_level_walk_batch(scene.h, C.byref(o), C.byref(b), fl.ctypes.data, None if st is None else st.ctypes.data,
                                      pre.ctypes.data, post.ctypes.data, float(margin), int(abs_int), stage.ctypes.data,
                                      counts.ctypes.data, accepted.ctypes.data, wave.ctypes.data, C.byref(n_waves), 0, None))
    return stage, counts, accepted, wave, int(n_waves.value)


def last_level_walk(scene: Scene):
    """(rounds, most rounds in one wave, in-order passes) of the last level_walk on this scene."""
    r, m, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _chk(lib().hpmvs_last_level_walk(scene.h, C.byref(r), C.byref(m), C.byref(f)))
    return int(r.value), int(m.value), int(f.value)


def build_pyramid(img: np.ndarray, device: int = 0) -> np.ndarray:
    h, w, _ = img.shape
    img = np.ascontiguousarray(img, dtype=np.uint8)
    out = np.zeros((h // 2, w // 2, 3), dtype=np.uint8)
    _chk(lib().hpmvs_build_pyramid(device, img.ctypes.data, w, h, out.ctypes.data, 0))
    return out


INT32_MAX = 2**31 - 1
REGULARIZE_PROBES = 24


def regularize_batch(scene: Scene, cells: Batch, cell_width, position, expanded, root_center, root_width, leaf_center,
                     leaf_width, leaf_patch, born=None, died=None, flatness=None, neighbours: bool = True):
    """CellProcessor::regularize (reference CellProcessor.cpp:309-367) for every cell against a versioned table of the nonempty
    leaves (include/hpmvs_amd.h: hpmvs_regularize_batch).  leaf_center / leaf_width: Leaf::c_ / width_, leaf_patch: the centre
    of data[0]; born / died (default: -1 / INT32_MAX, the tree as it is) the queue positions between which a leaf exists.
    flatness: the cells' flatness_ before the call (default -1), kept for unexpanded cells.
    Returns (flatness [n] float32, n_neighbours [n] int32 (-1: not expanded), neighbour_leaf [n, 24] int32 or None)."""
    n = cells.n
    L = int(len(leaf_width))
    cw = np.ascontiguousarray(cell_width, dtype=np.float32).reshape(n)
    pos = np.ascontiguousarray(position, dtype=np.int32).reshape(n)
    exp = np.ascontiguousarray(expanded).astype(np.uint8).reshape(n)
    lc = np.ascontiguousarray(leaf_center, dtype=np.float32).reshape(L, 3)
    lw = np.ascontiguousarray(leaf_width, dtype=np.float32).reshape(L)
    lp = np.ascontiguousarray(np.asarray(leaf_patch, dtype=np.float32)[:, :3]).reshape(L, 3)
    lb = np.full(L, -1, np.int32) if born is None else np.ascontiguousarray(born, dtype=np.int32).reshape(L)
    ld = np.full(L, INT32_MAX, np.int32) if died is None else np.ascontiguousarray(died, dtype=np.int32).reshape(L)
    t = LeafTable()
    t.n = L
    for k in range(3):
        t.root_center[k] = float(np.float32(root_center[k]))
    t.root_width = float(np.float32(root_width))
    t.cell_center, t.cell_width, t.patch_center = lc.ctypes.data, lw.ctypes.data, lp.ctypes.data
    t.born, t.died = lb.ctypes.data, ld.ctypes.data
    fl = np.full(n, -1.0, np.float32) if flatness is None else np.ascontiguousarray(flatness, dtype=np.float32).reshape(n).copy()
    nn = np.zeros(n, np.int32)
    nb = np.zeros((n, REGULARIZE_PROBES), np.int32) if neighbours else None
    b = cells.c_struct()
    _chk(lib().hpmvs_regularize_batch(scene.h, C.byref(b), cw.ctypes.data, pos.ctypes.data, exp.ctypes.data, C.byref(t),
                                      fl.ctypes.data, nn.ctypes.data, None if nb is None else nb.ctypes.data, 0, None))
    return fl, nn, nb


def filter_batch(scene: Scene, patches: Batch, cell_start):
    """CellProcessor::filter (reference CellProcessor.cpp:43-82) for every cell (include/hpmvs_amd.h: hpmvs_filter_batch): cell c
    holds the rows cell_start[c] .. cell_start[c + 1] - 1 of `patches`, in data order.  Returns (dist [n] float32, keep [n_cells]
    int32: the kept row, -1 for an empty cell, -2 for a cell with no winner)."""
    cs = np.ascontiguousarray(cell_start, dtype=np.int32).reshape(-1)
    if len(cs) < 1:
        raise ValueError("filter_batch: cell_start needs n_cells + 1 entries")
    dist = np.zeros(patches.n, np.float32)
    keep = np.zeros(len(cs) - 1, np.int32)
    b = patches.c_struct()
    _chk(lib().hpmvs_filter_batch(scene.h, C.byref(b), cs.ctypes.data, len(cs) - 1, dist.ctypes.data, keep.ctypes.data, 0, None))
    return dist, keep


def seed_tree_batch(scene: Scene, batch: Batch, patch_init_maxlevel: int = 9, set_depths: bool = True):
    """The second half of Scene::initPatches (reference Scene.cpp:183-199) for the rows of `batch` with ok != 0, in row order
    (include/hpmvs_amd.h: hpmvs_seed_tree_batch): bounding box, root, the scale floor (batch.scale is updated in place), the octree
    of the sequential patchTree_.add loop and, with set_depths, setDepths of the same rows.  Returns (SeedTreeInfo, rows [n],
    cell_start [n + 1], cell_center [n, 3], cell_width [n], cell_level [n], patch_center [n, 3]), zero from n_rows / n_leaves on."""
    n = batch.n
    info = SeedTreeInfo()
    rows = np.zeros(n, np.int32); cs = np.zeros(n + 1, np.int32)
    cc = np.zeros((n, 3), np.float32); cw = np.zeros(n, np.float32); cl = np.zeros(n, np.int32); pc = np.zeros((n, 3), np.float32)
    b = batch.c_struct()
    _chk(lib().hpmvs_seed_tree_batch(scene.h, C.byref(b), int(patch_init_maxlevel), int(bool(set_depths)), C.byref(info),
                                     rows.ctypes.data, cs.ctypes.data, cc.ctypes.data, cw.ctypes.data, cl.ctypes.data,
                                     pc.ctypes.data, 0, None))
    return info, rows, cs, cc, cw, cl, pc


OCTREE_MAX_DEPTH = 21   # HPMVS_MAX_TREE_DEPTH: levels of a path key
OCTREE_OUTPUTS = ("inside", "leaf_key", "leaf_index", "leaf_width", "leaf_center", "target_key")


@dataclass
class OctreeLocation:
    inside: np.ndarray             # [n] uint8 root.contains(p)
    leaf_key: np.ndarray           # [n] uint64 path key of the leaf root->at(p)
    leaf_index: np.ndarray         # [n] int32 index into the leaf keys given, -1: an empty leaf
    leaf_width: np.ndarray         # [n] float32
    leaf_center: np.ndarray        # [n, 3] float32
    target_key: np.ndarray         # [n] uint64 addConditional's leaf, 0: refused (or no add_width)


def _octree_index(root_center, root_width, bk, lk) -> OctreeIndex:
    t = OctreeIndex()
    for k in range(3):
        t.root_center[k] = float(np.float32(root_center[k]))
    t.root_width = float(np.float32(root_width))
    t.n_branches, t.n_leaves = len(bk), len(lk)
    t.branch_key, t.leaf_key = bk.ctypes.data, lk.ctypes.data
    return t


def _points3(points) -> np.ndarray:
    pts = np.asarray(points, dtype=np.float32)
    return np.ascontiguousarray(pts.reshape(-1, pts.shape[-1] if pts.ndim > 1 else 3)[:, :3])   # [n, 3] or [n, 4] centres


def octree_locate_batch(scene: Scene, root_center, root_width, branch_key, leaf_key, points, add_width=None) -> OctreeLocation:
    """root->at(p), getRoot()->contains(p) and DynOctTree::addConditional's target for every point against an octree given as
    path keys (include/hpmvs_amd.h: hpmvs_octree_locate_batch): branch_key the branches below the root, leaf_key the nonempty
    leaves.  add_width: a scalar or [n] (None: no target keys).  HpmvsError when the keys are no tree."""
    bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
    lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
    pts = _points3(points)
    n = len(pts)
    aw = None if add_width is None else np.ascontiguousarray(np.broadcast_to(np.asarray(add_width, dtype=np.float32), (n,)))
    t = _octree_index(root_center, root_width, bk, lk)
    r = OctreeLocation(np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.float32),
                       np.zeros((n, 3), np.float32), np.zeros(n, np.uint64))
    _chk(lib().hpmvs_octree_locate_batch(scene.h, C.byref(t), n, pts.ctypes.data, None if aw is None else aw.ctypes.data,
                                         *[getattr(r, k).ctypes.data for k in OCTREE_OUTPUTS], 0, None))
    return r


EXTEND_TREE_KEYS = ("skip", "pre_inside", "pre_key", "border", "post_key")


@dataclass
class ExtendTreeKeys:
    skip: np.ndarray               # [6 n] uint8 pre-gated by the tree (CellProcessor.cpp:124): built, not refined, stage 20
    pre_inside: np.ndarray         # [6 n] uint8 root.contains(centre before optimize)
    pre_key: np.ndarray            # [6 n] uint64 inside: addConditional's target leaf (0: refused); outside: 0
    border: np.ndarray             # [6 n] uint8 refined (ok != 0) and outside the root (:147)
    post_key: np.ndarray           # [6 n] uint64 refined and inside: the target leaf (0: refused); else 0

    def c_struct(self) -> ExtendTreeKeysStruct:
        k = ExtendTreeKeysStruct()
        for name in EXTEND_TREE_KEYS:
            setattr(k, name, _ptr(getattr(self, name)))
        return k


def extend_tree_batch(scene: Scene, parents: Batch, width, root_center, root_width, branch_key, leaf_key,
                      options: Options | None = None):
    """The candidate steps of one extend level against the real octree as ONE hpmvs_extend_tree_batch (include/hpmvs_amd.h):
    the six candidates of every parent built, looked up in the tree given as path keys, refined unless the tree pre-gates them,
    gated, and the refined ones looked up again.  `width`: the leaf width of the level, an exact level width of the tree
    (HpmvsError otherwise, as when the keys are no tree).  Returns (out: Batch of 6 n candidates, ExtendTreeKeys)."""
    o = options or default_options()
    bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
    lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
    t = _octree_index(root_center, root_width, bk, lk)
    N = 6 * parents.n
    out = Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                np.full((N, parents.max_images), -1, np.int32))
    keys = ExtendTreeKeys(np.zeros(N, np.uint8), np.zeros(N, np.uint8), np.zeros(N, np.uint64), np.zeros(N, np.uint8),
                          np.zeros(N, np.uint64))
    pb, ob, kb = parents.c_struct(), out.c_struct(), keys.c_struct()
    _chk(lib().hpmvs_extend_tree_batch(scene.h, C.byref(o), C.byref(t), C.byref(pb), float(np.float32(width)), C.byref(ob),
                                       C.byref(kb), 0, None))
    return out, keys


def octree_forest(roots, branch_first, leaf_first, branch_key, leaf_key):
    """The C structure of a forest (include/hpmvs_amd.h: hpmvs_octree_forest) over contiguous copies of the arrays given:
    roots [n_trees, 4] (c_, width_), the offsets [n_trees + 1] and the concatenated keys.  Returns (OctreeForest, arrays): keep
    `arrays` alive while the structure is in use."""
    rt = np.ascontiguousarray(np.asarray(roots, dtype=np.float32).reshape(-1, 4))
    bf = np.ascontiguousarray(branch_first, dtype=np.int32).reshape(-1)
    lf = np.ascontiguousarray(leaf_first, dtype=np.int32).reshape(-1)
    bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
    lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
    if len(bf) != len(rt) + 1 or len(lf) != len(rt) + 1:
        raise ValueError("octree_forest: branch_first / leaf_first need n_trees + 1 entries")
    if len(bk) != max(int(bf[-1]), 0) or len(lk) != max(int(lf[-1]), 0):
        raise ValueError("octree_forest: the last offset must be the number of keys given")
    f = OctreeForest()
    f.n_trees = len(rt)
    f.root, f.branch_first, f.leaf_first = rt.ctypes.data, bf.ctypes.data, lf.ctypes.data
    f.branch_key, f.leaf_key = bk.ctypes.data, lk.ctypes.data
    return f, (rt, bf, lf, bk, lk)


def extend_forest_batch(scene: Scene, parents: Batch, parent_tree, width, roots, branch_first, leaf_first, branch_key, leaf_key,
                        options: Options | None = None):
    """extend_tree_batch for ALL trees of a forest as ONE hpmvs_extend_forest_batch (include/hpmvs_amd.h): tree k has the root
    roots[k] (c_, width_) and the keys branch_key[branch_first[k]:branch_first[k + 1]] / leaf_key[leaf_first[k]:leaf_first[k + 1]],
    relative to its own root; parent_tree[i] names the tree of parent i, in any order.  Rows 6 i .. 6 i + 5 equal what
    extend_tree_batch returns for that tree alone.  HpmvsError names the offending tree.  Returns (out, ExtendTreeKeys)."""
    o = options or default_options()
    f, hold = octree_forest(roots, branch_first, leaf_first, branch_key, leaf_key)
    pt = np.ascontiguousarray(parent_tree, dtype=np.int32).reshape(-1)
    if len(pt) != parents.n:
        raise ValueError("extend_forest_batch: parent_tree needs one entry per parent")
    N = 6 * parents.n
    out = Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                np.full((N, parents.max_images), -1, np.int32))
    keys = ExtendTreeKeys(np.zeros(N, np.uint8), np.zeros(N, np.uint8), np.zeros(N, np.uint64), np.zeros(N, np.uint8),
                          np.zeros(N, np.uint64))
    pb, ob, kb = parents.c_struct(), out.c_struct(), keys.c_struct()
    _chk(lib().hpmvs_extend_forest_batch(scene.h, C.byref(o), C.byref(f), C.byref(pb), pt.ctypes.data, float(np.float32(width)),
                                         C.byref(ob), C.byref(kb), 0, None))
    del hold
    return out, keys


PROCESS_FOREST_OUTPUTS = ("support", "removed", "split", "children", "child_key", "n_neighbours", "neighbour_key")


@dataclass
class ProcessForestResult:
    candidates: Batch              # the 4 n branch children (stage 20: not built / not refined)
    flatness: np.ndarray           # [n] float32 flatness_ after the sweep (regularized cells updated, the others as given)
    support: np.ndarray            # [n] int32 Scene::getLevelSupport of every cell's patch
    removed: np.ndarray            # [n] uint8 flatness_ > 2.4: the patch was removed
    split: np.ndarray              # [n] uint8 the leaf was split
    children: np.ndarray           # [n, 4] uint8 the children that go into the new leaves
    child_key: np.ndarray          # [n, 4] uint64 the key (in the cell's tree) of the leaf child k went into, 0: none
    n_neighbours: np.ndarray       # [n] int32 neighbour leaves of the regularized cells, -2: settled
    neighbour_key: np.ndarray      # [n, 24] uint64 their keys in the cell's tree, first-probe order, 0-padded (None unless asked for)

    def c_struct(self) -> ProcessForestResultStruct:
        r = ProcessForestResultStruct()
        for name in PROCESS_FOREST_OUTPUTS:
            setattr(r, name, _ptr(getattr(self, name)))
        return r


def process_forest_batch(scene: Scene, cells: Batch, cell_tree, cell_key, flatness, final_level, roots, branch_first, leaf_first,
                         branch_key, leaf_key, leaf_patch_center, options: Options | None = None,
                         neighbours: bool = False) -> ProcessForestResult:
    """One regularize / settle sweep of processCell over the cells of ALL trees of a forest, in row order, as ONE
    hpmvs_process_forest_batch (include/hpmvs_amd.h): cell i is data[0] of the nonempty leaf cell_key[i] of tree cell_tree[i];
    leaf_patch_center [all leaves, 3] is data[0]->center_ of every nonempty leaf in leaf_key order.  The depth maps of the scene
    are updated; the keys given are not changed.  HpmvsError names the offending tree or cell; nothing is written then."""
    o = options or default_options()
    f, hold = octree_forest(roots, branch_first, leaf_first, branch_key, leaf_key)
    n = cells.n
    ct = np.ascontiguousarray(cell_tree, dtype=np.int32).reshape(-1)
    ck = np.ascontiguousarray(cell_key, dtype=np.uint64).reshape(-1)
    fl = np.array(flatness, dtype=np.float32).reshape(-1)
    fin = np.ascontiguousarray(np.asarray(final_level).astype(np.uint8)).reshape(-1)
    pc = np.ascontiguousarray(np.asarray(leaf_patch_center, dtype=np.float32).reshape(-1, 3))
    if not len(ct) == len(ck) == len(fl) == len(fin) == n:
        raise ValueError("process_forest_batch: cell_tree / cell_key / flatness / final_level need one entry per cell")
    if len(pc) != len(hold[4]):
        raise ValueError("process_forest_batch: leaf_patch_center needs one row per leaf key")
    N = 4 * n
    out = Batch(np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32),
                np.full((N, cells.max_images), -1, np.int32))
    r = ProcessForestResult(out, fl, np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8),
                            np.zeros((n, 4), np.uint64), np.zeros(n, np.int32),
                            np.zeros((n, REGULARIZE_PROBES), np.uint64) if neighbours else None)
    cb, ob, rb = cells.c_struct(), out.c_struct(), r.c_struct()
    _chk(lib().hpmvs_process_forest_batch(scene.h, C.byref(o), C.byref(f), pc.ctypes.data, C.byref(cb), ct.ctypes.data, ck.ctypes.data,
                                          fl.ctypes.data, fin.ctypes.data, C.byref(ob), C.byref(rb), 0, None))
    del hold
    return r


@dataclass
class OctreeInsertion:
    accepted: np.ndarray           # [n] uint8 addConditional's return, in queue order
    leaf_key: np.ndarray           # [n] uint64 *outleaf: the leaf the patch went into, or the one that refused it
    blocker: np.ndarray            # [n] int32 queue index of the earlier patch behind a refusal, -1: accepted, or refused by the tree


def octree_insert_batch(scene: Scene, root_center, root_width, branch_key, leaf_key, points, add_width) -> OctreeInsertion:
    """DynOctTree::addConditional(points[i], add_width[i]) for i = 0 .. n - 1 in that order against the octree given as path
    keys, every patch seeing the earlier ones' leaves (include/hpmvs_amd.h: hpmvs_octree_insert_batch; the insertion loop of
    CellProcessor::processBorderCellQueue).  The keys given are not changed: the caller enters the accepted ones."""
    bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
    lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
    pts = _points3(points)
    n = len(pts)
    aw = np.ascontiguousarray(np.broadcast_to(np.asarray(add_width, dtype=np.float32), (n,)))
    t = _octree_index(root_center, root_width, bk, lk)
    r = OctreeInsertion(np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int32))
    _chk(lib().hpmvs_octree_insert_batch(scene.h, C.byref(t), n, pts.ctypes.data, aw.ctypes.data, r.accepted.ctypes.data,
                                         r.leaf_key.ctypes.data, r.blocker.ctypes.data, 0, None))
    return r


def octree_route_batch(scene: Scene, roots, points) -> np.ndarray:
    """For every point the index of the first root in list order (roots [n_trees, 4]: c_, width_) whose Cell::contains holds,
    -1 when none does (include/hpmvs_amd.h: hpmvs_octree_route_batch; CellProcessor::distributeBorderCell)."""
    rt = np.ascontiguousarray(np.asarray(roots, dtype=np.float32).reshape(-1, 4))
    pts = _points3(points)
    tree = np.zeros(len(pts), np.int32)
    _chk(lib().hpmvs_octree_route_batch(scene.h, len(rt), rt.ctypes.data, len(pts), pts.ctypes.data, tree.ctypes.data, 0, None))
    return tree


@dataclass
class BorderForestInsertion:
    tree: np.ndarray               # [n] int32 the first tree in list order whose root contains the patch, -1: none (dropped)
    accepted: np.ndarray           # [n] uint8 addConditional's return in that tree, in queue order
    leaf_key: np.ndarray           # [n] uint64 the key in that tree of the leaf the patch went into, or that refused it; 0: dropped
    blocker: np.ndarray            # [n] int32 queue index of the earlier patch behind a refusal, -1: accepted, refused by the tree, dropped

    def c_struct(self) -> BorderForestResultStruct:
        r = BorderForestResultStruct()
        r.tree, r.accepted, r.leaf_key, r.blocker = _ptr(self.tree), _ptr(self.accepted), _ptr(self.leaf_key), _ptr(self.blocker)
        return r


def border_forest_batch(scene: Scene, border: Batch, roots, branch_first, leaf_first, branch_key, leaf_key,
                        set_depths: bool = True) -> BorderForestInsertion:
    """A round's border queue delivered to ALL trees of a forest as ONE hpmvs_border_forest_batch (include/hpmvs_amd.h):
    octree_route_batch over `roots`, then for every tree octree_insert_batch of its rows in queue order with add_width =
    scale * 2.0, then set_depths_batch over the accepted rows (set_depths).  The forest is given as extend_forest_batch takes
    it; the keys are not changed: the caller enters the accepted ones.  HpmvsError names the offending tree; nothing is
    written then."""
    f, hold = octree_forest(roots, branch_first, leaf_first, branch_key, leaf_key)
    n = border.n
    r = BorderForestInsertion(np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int32))
    bb, rb = border.c_struct(), r.c_struct()
    _chk(lib().hpmvs_border_forest_batch(scene.h, C.byref(f), C.byref(bb), 1 if set_depths else 0, C.byref(rb), 0, None))
    del hold
    return r


MAX_SUBTREES = 4096   # HPMVS_MAX_SUBTREES: the largest min_trees
PARTITION_STOP = ("the root alone", "the list reached min_trees", "the largest subtree is below min_split_leaves")
PARTITION_OUTPUTS = ("root_key", "root_cell", "tree_first", "tree_leaves", "leaf_order", "leaf_tree", "leaf_sub_key", "branch_tree",
                     "branch_sub_key")


@dataclass
class OctreePartition:
    n_trees: int
    n_orphans: int                 # nonempty leaves in no subtree
    n_splits: int                  # iterations of getSubTrees' while loop that cut a subtree
    stop: int                      # index into PARTITION_STOP
    histogram: np.ndarray          # [22] int32 cellHistogram: nonempty leaves by depth below the root
    root_key: np.ndarray           # [cap] uint64 the subtree roots in the reference's list order, 0 from n_trees on
    root_cell: np.ndarray          # [cap, 4] float32 c_, width_
    tree_first: np.ndarray         # [cap] int32 subtree k's nonempty leaves: leaf_order[tree_first[k] : tree_first[k] + tree_leaves[k]]
    tree_leaves: np.ndarray        # [cap] int32
    leaf_order: np.ndarray         # [n_leaves] int32 indices into the leaf keys given, in Leaf_iterator order
    leaf_tree: np.ndarray          # [n_leaves] int32 -1: an orphan
    leaf_sub_key: np.ndarray       # [n_leaves] uint64 the key re-based on its subtree's root, 0 for an orphan
    branch_tree: np.ndarray        # [n_branches] int32 -1: a root or a branch above the roots
    branch_sub_key: np.ndarray     # [n_branches] uint64


def partition_capacity(min_trees: int) -> int:
    """Entries of the root outputs of hpmvs_octree_partition: the list cannot end longer."""
    return max(8, int(min_trees) + 6)


def octree_partition(scene: Scene, root_center, root_width, branch_key, leaf_key, min_trees: int = 100,
                     min_split_leaves: int = 100) -> OctreePartition:
    """getSubTrees(tree, list, min_trees) of the reference's main (src/main.cpp:50-96) and DynOctTree::cellHistogram for an octree
    given as path keys in any order, as ONE call (include/hpmvs_amd.h: hpmvs_octree_partition).  min_split_leaves is the
    reference's constant 100.  HpmvsError when the keys are no tree, min_trees > MAX_SUBTREES or min_split_leaves < 1."""
    bk = np.ascontiguousarray(branch_key, dtype=np.uint64).reshape(-1)
    lk = np.ascontiguousarray(leaf_key, dtype=np.uint64).reshape(-1)
    t = _octree_index(root_center, root_width, bk, lk)
    cap, nb, nl = partition_capacity(min_trees), len(bk), len(lk)
    info = OctreePartitionInfo()
    r = OctreePartition(0, 0, 0, 0, np.zeros(22, np.int32), np.zeros(cap, np.uint64), np.zeros((cap, 4), np.float32),
                        np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(nl, np.int32), np.zeros(nl, np.int32),
                        np.zeros(nl, np.uint64), np.zeros(nb, np.int32), np.zeros(nb, np.uint64))
    _chk(lib().hpmvs_octree_partition(scene.h, C.byref(t), int(min_trees), int(min_split_leaves), C.byref(info),
                                      *[getattr(r, k).ctypes.data for k in PARTITION_OUTPUTS], 0, None))
    r.n_trees, r.n_orphans, r.n_splits, r.stop = info.n_trees, info.n_orphans, info.n_splits, info.stop
    r.histogram[:] = info.histogram[:]
    return r


PLY_BINARY, PLY_NORMAL, PLY_SCALE, PLY_VISIBILITY = 1, 2, 4, 8   # HPMVS_PLY_*


def ply_flags(binary=False, normal=True, scale=True, visibility=True) -> int:
    return (PLY_BINARY if binary else 0) | (PLY_NORMAL if normal else 0) | (PLY_SCALE if scale else 0) | \
        (PLY_VISIBILITY if visibility else 0)


def ply_ext(batch: Batch, order=None, binary=False, normal=True, scale=True, visibility=True, device: int = 0) -> np.ndarray:
    """The file the reference's DynOctTree::toExtPly writes (include/hpmvs/doctree.h:526-622; the defaults are its own, ASCII) for
    the rows `order` of the batch -- None: all rows in order; a row may be named more than once -- as a uint8 array, header
    included: float-to-text conversion, the lines' placement and their writing run on the GPU (include/hpmvs_amd.h:
    hpmvs_ply_ext_batch).  Reads center, normal, scale, color, n_images, images; a batch whose arrays are device tensors is read
    in place (`order` then is a device tensor too).  Makes a size query first, then the call.  HpmvsError naming the row for an
    order entry outside the batch or an n_images outside [0, max_images]."""
    b = batch.c_struct()
    on_device = int(not isinstance(batch.center, np.ndarray))
    n_rows = 0
    if order is not None:
        if not on_device:
            order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        n_rows = int(order.shape[0])
        if n_rows == 0:   # (a NULL order means every row: an empty one still needs an address)
            order = np.zeros(1, dtype=np.int32) if not on_device else torch.zeros(1, dtype=torch.int32, device=order.device)
    flags = ply_flags(binary, normal, scale, visibility)
    n = C.c_size_t(0)
    _chk(lib().hpmvs_ply_ext_batch(device, C.byref(b), _ptr(order), n_rows, flags, None, 0, C.byref(n), on_device, None))
    out = np.empty(n.value, dtype=np.uint8)
    _chk(lib().hpmvs_ply_ext_batch(device, C.byref(b), _ptr(order), n_rows, flags, out.ctypes.data, out.nbytes, C.byref(n), on_device, None))
    return out[:n.value]


def write_ext_ply(path, batch: Batch, order=None, binary=False, normal=True, scale=True, visibility=True, device: int = 0) -> int:
    """ply_ext's bytes as the file `path`; returns their number."""
    data = ply_ext(batch, order, binary, normal, scale, visibility, device)
    with open(path, "wb") as f:
        f.write(data.tobytes())
    return int(data.size)
