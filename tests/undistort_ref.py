"""Host restatement of the level-0 undistortion (tests/undistort_host.cpp over hpmvs_amd/csrc/undistort.hpp), built
with g++ -std=c++11 -O2 -ffp-contract=off into a directory the caller chooses and loaded through ctypes.  No numpy
arithmetic: pow / complex must be glibc's, as in the reference."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "undistort_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g6_undistort.npz")


class HostUndistort:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libundistort_host.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", SRC, "-o", so],
                       check=True, capture_output=True)
        L = C.CDLL(so)
        L.ud_map.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
        L.ud_map.restype = None
        L.ud_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int]
        L.ud_image.restype = None
        self.L = L

    def map(self, w, h, f, k1):
        xy = np.empty((h, w, 2), dtype=np.float32)
        self.L.ud_map(w, h, float(f), float(k1), xy.ctypes.data)
        return xy

    def image(self, img, f, k1, threads=1):
        """-> (undistorted u8 [H, W, 3] with 0 where unwritten, written mask [H, W] bool)"""
        src = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, _ = src.shape
        out = np.empty_like(src)
        written = np.empty((h, w), dtype=np.uint8)
        self.L.ud_image(src.ctypes.data, w, h, float(f), float(k1), out.ctypes.data, written.ctypes.data, int(threads))
        return out, written.astype(bool)


def golden_cases():
    """[(input image, f, k1, reference output, written mask)] of tests/golden/g6_undistort.npz"""
    d = np.load(GOLDEN)
    out = []
    for n in range(len(d["cases_f"])):
        img = d[str(d["cases_image"][n]) + "_in"]
        out.append((img, float(d["cases_f"][n]), float(d["cases_k1"][n]), d[f"case{n}_out"], d[f"case{n}_written"]))
    return out
