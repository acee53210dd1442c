"""Host restatement of the parallel JPEG entropy decode (tests/jpeg_entropy_host.cpp over hpmvs_amd/csrc/jpeg.hpp), built
with g++ into a directory the caller chooses and loaded through ctypes, and the files of tests/golden/g8_jpeg_entropy.npz
(made by tests/golden/make_golden_jpeg_entropy.py with Pillow; no test imports Pillow) together with g7's."""
import ctypes as C
import os
import subprocess

import numpy as np

from jpeg_ref import Golden, mutations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "jpeg_entropy_host.cpp")
GOLDEN8 = os.path.join(ROOT, "tests", "golden", "g8_jpeg_entropy.npz")
SHIPPED_BITS = 512                                   # jpeg.hpp: kSubseqBits
SWEEP = list(range(64, 257, 32)) + [SHIPPED_BITS]    # subsequence sizes every file is decoded at
HOST, DEVICE = 1, 2                                  # HPMVS_JPEG_ENTROPY_HOST / _DEVICE


def files():
    """[(name, bytes)]: g8's seven files and g7's thirteen, in a fixed order"""
    d = np.load(GOLDEN8)
    g7 = Golden()
    return [(str(n), d[str(n) + "_jpg"].tobytes()) for n in d["names"]] + [(n, g7.jpg[n]) for n in g7.names]


def mutation_set():
    """[(name, index of the mutation, bytes)]: jpeg_ref.mutations(data, seed=index of the file, 60, 6) of every file"""
    return [(n, k, m) for i, (n, b) in enumerate(files()) for k, m in enumerate(mutations(b, i, 60, 6))]


class EntropyHost:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libjpeg_entropy_host.so")
        subprocess.run(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", SRC, "-o", so], check=True, capture_output=True)
        L = C.CDLL(so)
        L.je_n_coef.restype = C.c_size_t
        L.je_n_coef.argtypes = [C.c_char_p, C.c_size_t]
        L.je_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int]
        L.je_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.c_char_p, C.c_int]
        self.L = L

    def host(self, data):
        """decode_file -> (code, int16 coefficients or None, message)"""
        n = self.L.je_n_coef(data, len(data))
        coef = np.zeros(max(n, 1), np.int16)
        err = C.create_string_buffer(256)
        rc = self.L.je_host(data, len(data), coef.ctypes.data, n, err, 256)
        return rc, coef[:n] if rc == 0 else None, err.value.decode()

    def scheme(self, data, subseq_bits=0, round_cap=0):
        """the parallel scheme with its fallback -> (code, coefficients or None, message, accepted, rounds)"""
        n = self.L.je_n_coef(data, len(data))
        coef = np.zeros(max(n, 1), np.int16)
        err = C.create_string_buffer(256)
        used, rounds = C.c_int(), C.c_int()
        rc = self.L.je_decode(data, len(data), subseq_bits, round_cap, coef.ctypes.data, n, C.byref(used), C.byref(rounds), err, 256)
        return rc, coef[:n] if rc == 0 else None, err.value.decode(), bool(used.value), rounds.value
