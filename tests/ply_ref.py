"""What the PLY tests share: the file of the reference's DynOctTree::toExtPly (include/hpmvs/doctree.h:526-622) built by Python
formatting, the values the contract lists, synthetic batches, and the host restatement of hpmvs_amd/csrc/ply_text.hpp.

The pin is this machine's C library: Python's '%.6g' % float(np.float32(v)) and snprintf("%.6g") both print the exact binary
value (glibc), as libstdc++'s operator<<(float) does.  No file written by the reference itself can be a fixture: its
translation units need Eigen, which is not available where the fixtures are made."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ply_text_host.cpp")
BINARY, NORMAL, SCALE, VISIBILITY = 1, 2, 4, 8

# value -> text, as the contract states them
CONTRACT = [
    (1234565.0, "1.23456e+06"), (1234575.0, "1.23458e+06"), (1024.125, "1024.12"), (1024.375, "1024.38"),
    (999999.5, "1e+06"), (999999.4, "999999"), (9.9999995, "10"), (0.0001, "0.0001"), (1e-5, "1e-05"),
    (-0.0, "-0"), (0.0, "0"), (math.inf, "inf"), (-math.inf, "-inf"), (1e-45, "1.4013e-45"),
]
NANS = [(0x7FC00000, "nan"), (0xFFC00000, "-nan"), (0x7F800001, "nan"), (0xFFFFFFFF, "-nan")]


def special_bits() -> np.ndarray:
    """The contract's values, both NaN signs, the extremes of the format and a few 12-character texts, as bit patterns."""
    v = np.array([c[0] for c in CONTRACT] + [-1.17549435e-38, 3.4028235e38, -3.4028235e38, -0.000123457, -1.23457e-5, 1.0, -1.0,
                                             0.5, 123000.0, 100000.0, 0.1, -1e-44], dtype=np.float32)
    return np.concatenate([v.view(np.uint32), np.array([b for b, _ in NANS], dtype=np.uint32)])


def fmt(v) -> str:
    """ostream << float / printf("%.6g") of a float32, by Python (glibc prints -nan for a NaN with the sign bit; Python does not)."""
    f = np.float32(v)
    if np.isnan(f):
        return "-nan" if (int(f.view(np.uint32)) >> 31) else "nan"
    return "%.6g" % float(f)


def colour(v) -> int:
    """(unsigned char) of a value in [0, 256); outside: clamped, a NaN 0 (the product's documented rule)."""
    f = float(np.float32(v))
    if math.isnan(f) or f < 0:
        return 0
    return 255 if f >= 256 else int(f)


def header(n_rows: int, flags: int) -> bytes:
    h = ["ply", "format binary_little_endian 1.0" if flags & BINARY else "format ascii 1.0", f"element vertex {n_rows}",
         "property float x", "property float y", "property float z"]
    if flags & NORMAL:
        h += ["property float nx", "property float ny", "property float nz"]
    h += ["property uchar red", "property uchar green", "property uchar blue"]
    if flags & SCALE:
        h += ["property float scalar_scale"]
    if flags & VISIBILITY:
        h += [f"element point_visibility {n_rows}", "property list uint uint visible_cameras"]
    return ("\n".join(h + ["end_header"]) + "\n").encode()


def build(batch, order, flags: int) -> bytes:
    """The file for the rows `order` (None: all) of a batch with numpy arrays center [n][4], normal [n][4], scale, color [n][3],
    n_images, images."""
    rows = range(batch.n) if order is None else [int(r) for r in order]
    out = [header(len(rows), flags)]
    for p in rows:
        c, nr, col, s = batch.center[p], batch.normal[p], batch.color[p], batch.scale[p]
        rgb = [colour(col[k]) for k in range(3)]
        if flags & BINARY:
            rec = c[:3].astype("<f4").tobytes()   # (tobytes keeps a NaN's payload)
            if flags & NORMAL:
                rec += nr[:3].astype("<f4").tobytes()
            rec += bytes(rgb)
            if flags & SCALE:
                rec += np.float32(s).astype("<f4").tobytes()
            out.append(rec)
        else:
            f = [fmt(c[k]) for k in range(3)]
            if flags & NORMAL:
                f += [fmt(nr[k]) for k in range(3)]
            f += [str(k) for k in rgb]
            if flags & SCALE:
                f.append(fmt(s))
            out.append((" ".join(f) + " \n").encode())
    if flags & VISIBILITY:
        for p in rows:
            n = int(batch.n_images[p])
            ids = batch.images[p, :n].astype(np.uint32)
            if flags & BINARY:
                out.append(np.uint32(n).astype("<u4").tobytes() + ids.astype("<u4").tobytes())
            else:
                out.append((" ".join([str(n)] + [str(int(i)) for i in ids]) + " \n").encode())
    return b"".join(out)


class Rows:
    """The arrays of a batch the file is made from (what api.Batch holds, without the library)."""

    def __init__(self, n: int, max_images: int = 64, seed: int = 0):
        rng = np.random.default_rng(seed)
        sp = special_bits()
        pick = lambda shape: np.where(rng.random(shape) < 0.3, sp[rng.integers(0, len(sp), shape)],
                                      (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 8, shape)).astype(np.float32).view(np.uint32))
        self.n, self.max_images = n, max_images
        self.center = pick((n, 4)).astype(np.uint32).view(np.float32)
        self.normal = pick((n, 4)).astype(np.uint32).view(np.float32)
        self.scale = pick((n,)).astype(np.uint32).view(np.float32)
        cols = np.array([0.0, 0.99, 1.0, 17.99, 128.5, 255.0, 255.99, 256.0, 1e9, -3.0, np.nan, np.inf, -np.inf, 9.5, 99.9, 100.0], np.float32)
        self.color = cols[rng.integers(0, len(cols), (n, 3))]
        self.n_images = np.array([0, 1, 2, 7, 64], np.int32)[rng.integers(0, 5, n)]
        self.n_images = np.minimum(self.n_images, max_images).astype(np.int32)
        ids = np.array([0, 9, 10, 99, 100, 255, -1, 3, 42, 12345], np.int32)
        self.images = ids[rng.integers(0, len(ids), (n, max_images))]
        if n > 0:   # the shortest line there is: "0 0 0 0 0 0 0 0 0 0 \n"
            self.center[0] = 0; self.normal[0] = 0; self.scale[0] = 0; self.color[0] = 0; self.n_images[0] = 0
        if n > 1:   # ... and the longest: seven 12-character floats and three 3-digit colours
            self.center[1] = np.float32(-1.17549435e-38); self.normal[1] = np.float32(-0.000123457); self.scale[1] = np.float32(-1.23457e-5)
            self.color[1] = 255.0; self.n_images[1] = max_images


class HostPlyText:
    """tests/ply_text_host.cpp built with g++: ply_text.hpp's host compile."""

    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libply_text_host.so")
        subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        L = C.CDLL(so)
        L.pt_format.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.pt_format.restype = C.c_long
        L.pt_check_snprintf.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
        L.pt_check_snprintf.restype = C.c_long
        L.pt_check_list.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.pt_check_list.restype = C.c_long
        L.pt_colour_bytes.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.pt_file.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.pt_file.restype = C.c_size_t
        self.L = L

    def format(self, bits):
        """-> the texts of the floats with these bit patterns; asserts that float_len agrees with put_float"""
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        text = np.zeros((len(bits), 16), np.uint8)
        length = np.zeros(len(bits), np.int32)
        assert self.L.pt_format(bits.ctypes.data, len(bits), text.ctypes.data, length.ctypes.data) == 0
        return [bytes(t[:n]).decode() for t, n in zip(text, length)]

    def check_snprintf(self, first, stride, count):
        bad = C.c_uint32(0)
        return int(self.L.pt_check_snprintf(first, stride, count, C.byref(bad))), int(bad.value)

    def check_list(self, bits):
        """mismatches against snprintf("%.6g") among the floats with these bit patterns, and the first such pattern"""
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        bad = C.c_uint32(0)
        return int(self.L.pt_check_list(bits.ctypes.data, len(bits), C.byref(bad))), int(bad.value)

    def colour_bytes(self, values):
        bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
        out = np.zeros(len(bits), np.uint8)
        self.L.pt_colour_bytes(bits.ctypes.data, len(bits), out.ctypes.data)
        return out

    def file(self, rows, order, flags) -> bytes:
        a = [np.ascontiguousarray(x) for x in (rows.center, rows.normal, rows.scale, rows.color, rows.n_images, rows.images)]
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        n_rows = rows.n if o is None else len(o)
        args = [x.ctypes.data for x in a] + [rows.max_images, None if o is None else o.ctypes.data, n_rows, flags]
        n = self.L.pt_file(*args, None)
        out = np.zeros(max(1, n), np.uint8)
        assert self.L.pt_file(*args, out.ctypes.data) == n
        return out[:n].tobytes()
