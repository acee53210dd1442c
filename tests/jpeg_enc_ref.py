"""Host restatement of the baseline JPEG encode (tests/jpeg_enc_host.cpp over hpmvs_amd/csrc/jpeg_enc.hpp), built with g++
into a directory the caller chooses and loaded through ctypes, and the entries of tests/golden/g8_jpeg_enc.npz (made by
tests/golden/make_golden_jpeg_enc.py with Pillow; no test imports Pillow)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "jpeg_enc_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g8_jpeg_enc.npz")
HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED = 0, -2, -5
GUARD = 64
STATS = ("stuffed", "zrl", "dc_category", "pad_bits", "right_dummies", "bottom_dummies")


class HostJpegEnc:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libjpeg_enc_host.so")
        subprocess.run(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        L = C.CDLL(so)
        L.je_bound.argtypes = [C.c_int, C.c_int]
        L.je_bound.restype = C.c_size_t
        L.je_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p,
                                C.c_char_p, C.c_int]
        self.L = L

    def bound(self, w, h):
        return int(self.L.je_bound(w, h))

    def encode(self, rgb, quality, cap=None):
        """-> (code, file bytes or None, stats dict, message, guards intact); the output lies between two GUARD-byte
        fences of 0xA5 in a buffer of `cap` bytes (default: the bound)"""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w = rgb.shape[:2]
        cap = self.bound(w, h) if cap is None else cap
        raw = np.full(2 * GUARD + cap, 0xA5, np.uint8)
        n = C.c_size_t(0)
        stats = np.zeros(len(STATS), np.uint32)
        err = C.create_string_buffer(256)
        rc = self.L.je_encode(rgb.ctypes.data, w, h, quality, raw.ctypes.data + GUARD, cap, C.byref(n), stats.ctypes.data, err, 256)
        intact = bool((raw[:GUARD] == 0xA5).all() and (raw[GUARD + cap:] == 0xA5).all())
        if rc != 0 and n.value > cap:
            intact = intact and bool((raw[GUARD:GUARD + cap] == 0xA5).all())
        data = raw[GUARD:GUARD + n.value].tobytes() if rc == 0 else None
        return rc, data, dict(zip(STATS, (int(x) for x in stats))), err.value.decode(), intact


class Golden:
    def __init__(self):
        d = np.load(GOLDEN)
        self.pillow = str(d["pillow_version"])
        self.libjpeg = str(d["libjpeg_version"])
        self.names = [str(n) for n in d["names"]]
        self.quality = {n: int(q) for n, q in zip(self.names, d["quality"])}
        self.rgb = {n: d[str(i) + "_rgb"] for n, i in zip(self.names, d["input_of"])}   # (cases of one size and kind share an input)
        self.jpg = {n: d[n + "_jpg"].tobytes() for n in self.names}
        self.decoded = {str(n): d[str(n) + "_dec"] for n in d["decoded_names"]}   # Pillow's decode of the golden file
