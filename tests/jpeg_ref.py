"""Host restatement of the baseline JPEG decode (tests/jpeg_host.cpp over hpmvs_amd/csrc/jpeg.hpp), built with g++ into
a directory the caller chooses and loaded through ctypes, and the entries of tests/golden/g7_jpeg.npz (made by
tests/golden/make_golden_jpeg.py with Pillow; no test imports Pillow)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "jpeg_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g7_jpeg.npz")
HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_NODEVICE, HPMVS_ERR_UNSUPPORTED = 0, -2, -4, -5
GUARD = 64


class HostJpeg:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libjpeg_host.so")
        subprocess.run(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        L = C.CDLL(so)
        L.jh_info.argtypes = [C.c_char_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5 + [C.c_char_p, C.c_int]
        L.jh_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int]
        L.jh_nonzero_positions.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
        self.L = L

    def info(self, data):
        """-> (code, (w, h, components, h_samp, v_samp) or None, message)"""
        v = [C.c_int() for _ in range(5)]
        err = C.create_string_buffer(256)
        rc = self.L.jh_info(bytes(data), len(data), *[C.byref(x) for x in v], err, 256)
        return rc, tuple(x.value for x in v) if rc == 0 else None, err.value.decode()

    def decode_into(self, data, buf, cap):
        """decode into the address `buf` of `cap` bytes -> (code, message)"""
        err = C.create_string_buffer(256)
        rc = self.L.jh_decode(bytes(data), len(data), buf, cap, err, 256)
        return rc, err.value.decode()

    def decode(self, data, w, h):
        """-> (code, uint8 [h, w, 3] or None, guards intact); the output lies between two GUARD-byte fences of 0xA5"""
        raw = np.full(2 * GUARD + 3 * w * h, 0xA5, np.uint8)
        rc, _ = self.decode_into(data, raw.ctypes.data + GUARD, 3 * w * h)
        intact = bool((raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all())
        return rc, raw[GUARD:-GUARD].reshape(h, w, 3).copy() if rc == 0 else None, intact

    def nonzero_positions(self, data):
        counts = np.zeros(64, np.uint32)
        rc = self.L.jh_nonzero_positions(bytes(data), len(data), counts.ctypes.data)
        assert rc == 0, rc
        return counts


class Golden:
    def __init__(self):
        d = np.load(GOLDEN)
        self.pillow = str(d["pillow_version"])
        self.libjpeg = str(d["libjpeg_version"])
        self.names = [str(n) for n in d["names"]]
        self.info = {n: tuple(int(x) for x in d["info"][k]) for k, n in enumerate(self.names)}   # (w, h, components, h_samp, v_samp)
        self.jpg = {n: d[n + "_jpg"].tobytes() for n in self.names}
        self.rgb = {n: d[n + "_rgb"] for n in self.names}
        self.refuse_names = [str(n) for n in d["refuse_names"]]
        self.refuse_code = {n: int(c) for n, c in zip(self.refuse_names, d["refuse_codes"])}
        self.refuse_word = {n: str(w) for n, w in zip(self.refuse_names, d["refuse_words"])}
        self.refuse_jpg = {n: d[n + "_jpg"].tobytes() for n in self.refuse_names}
        self.scene_size = (int(d["scene_size"][0]), int(d["scene_size"][1]))
        self.scene_jpg = [d["scene_view%d_jpg" % i].tobytes() for i in range(int(d["scene_size"][2]))]


def mutations(data, seed, n_overwrites=200, n_cuts=20):
    """seeded single-byte overwrites and truncations of a file, in a fixed order"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_overwrites):
        b = bytearray(data)
        b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    for _ in range(n_cuts):
        out.append(bytes(data[: int(rng.integers(2, len(data)))]))
    return out
