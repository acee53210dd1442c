#!/usr/bin/env python3
"""Generates tests/golden/g6_undistort.npz IN THE BUILD CONTAINER from the reference's GENUINE Image::undistort
(src/hpmvs/Image.cpp:68-146 with its vendored CImg), compiled into a temporary directory together with the small
stand-ins below for the two headers the translation unit includes but undistort does not compute with
(<Eigen/Dense>: the repository's include/hpmvs/Vec.h; <glog/logging.h>: a null stream).  Data only is committed:
the input images, the undistorted level 0, and the mask of the pixels the reference actually wrote.

The mask: the reference leaves unwritten pixels as whatever `new float[]` held.  The driver replaces operator new[]
so that fresh blocks are filled with a float pattern, runs undistort twice with two patterns (17.0f and 230.0f, both
representable in u8) and marks as unwritten every pixel whose bytes differ between the two runs.

    python tests/golden/make_golden_undistort.py [REFERENCE_ROOT]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

EIGEN_STUB = r"""
#pragma once
#include <complex>
#define HPMVS_NO_EIGEN
#include <hpmvs/Vec.h>
namespace Eigen { typedef Matrix_<double, 2> Vector2d; }
"""

GLOG_STUB = r"""
#pragma once
#include <ostream>
struct NullStream : std::ostream { NullStream() : std::ostream(nullptr) {} };
inline std::ostream& null_stream() { static NullStream s; return s; }
#define LOG(x) null_stream()
#define VLOG(x) null_stream()
"""

DRIVER = r"""
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#define private public
#include <hpmvs/Image.h>
#undef private

static float g_fill = 0.0f;
void* operator new[](std::size_t n) {
    void* p = std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    float* f = (float*)p;
    for (std::size_t k = 0; k < n / sizeof(float); k++) f[k] = g_fill;
    return p;
}
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

// argv: in.bin out.bin w h f k1 fill    (interleaved u8 RGB in and out)
int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    const float f = (float)atof(argv[5]), k1 = (float)atof(argv[6]);
    std::vector<unsigned char> in((size_t)w * h * 3), out((size_t)w * h * 3);
    FILE* fi = fopen(argv[1], "rb");
    if (!fi || fread(in.data(), 1, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    mo3d::Image img;
    img.images_.resize(1);
    img.images_[0].assign(w, h, 1, 3);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) img.images_[0](x, y, 0, c) = in[3 * ((size_t)y * w + x) + c];
    img.f_ = f;
    img.k1_ = k1;
    g_fill = (float)atof(argv[7]);
    if (!img.undistort()) return 4;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) out[3 * ((size_t)y * w + x) + c] = img.images_[0](x, y, 0, c);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo || fwrite(out.data(), 1, out.size(), fo) != out.size()) return 5;
    fclose(fo);
    return 0;
}
"""

K1S = [1e-3, 0.05, 0.3, -0.05, -0.3, -1.0]
IMAGES = [("a", 120, 160, "rand"), ("b", 97, 161, "rand"), ("c", 240, 320, "ramp"), ("d", 48, 64, "rand")]
F_FACTORS = [0.9, 1.0, 1.1, 1.2]


def inputs():
    rng = np.random.default_rng(0x556E6469)
    out = {}
    for name, h, w, kind in IMAGES:
        if kind == "rand":
            out[name] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            # stepped ramps and a checkerboard: the interpolated edges without a fixture of incompressible bytes
            out[name] = np.stack([(xx * 255 // (w - 1)) & 0xE0, (yy * 255 // (h - 1)) & 0xE0, ((xx // 16 + yy // 16) % 2) * 255],
                                 axis=-1).astype(np.uint8)
    return out


def cases():
    """(image name, f, k1) of every fixture, in a fixed order."""
    out = []
    for i, (name, h, w, _) in enumerate(IMAGES):
        for j, k1 in enumerate(K1S):
            f = float(np.float32(F_FACTORS[(i + j) % len(F_FACTORS)] * w))
            out.append((name, f, k1))
    return out


def build(ref, tmp):
    for sub, text in (("Eigen/Dense", EIGEN_STUB), ("glog/logging.h", GLOG_STUB), ("driver.cpp", DRIVER)):
        p = os.path.join(tmp, sub)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as fh:
            fh.write(text)
    exe = os.path.join(tmp, "ref_undistort")
    cimg = os.path.join(ref, "thirdLibs", "cimg")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Dcimg_display=0", "-include", os.path.join(cimg, "CImg.h"),
           "-I" + tmp, "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + cimg,
           os.path.join(tmp, "driver.cpp"), os.path.join(ref, "src", "hpmvs", "Image.cpp"), "-o", exe, "-lpthread"]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, tmp, img, f, k1, fill):
    h, w, _ = img.shape
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    img.tofile(fi)
    subprocess.run([exe, fi, fo, str(w), str(h), repr(f), repr(k1), repr(fill)], check=True)
    return np.fromfile(fo, dtype=np.uint8).reshape(h, w, 3)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ins = inputs()
    arrs = {f"{k}_in": v for k, v in ins.items()}
    meta = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref, tmp)
        for n, (name, f, k1) in enumerate(cases()):
            a = run(exe, tmp, ins[name], f, k1, 17.0)
            b = run(exe, tmp, ins[name], f, k1, 230.0)
            written = (a == b).all(axis=-1)
            arrs[f"case{n}_out"] = np.where(written[..., None], a, 0).astype(np.uint8)
            arrs[f"case{n}_written"] = written
            meta.append((name, f, k1))
            print(f"case {n}: {name} {ins[name].shape} f={f} k1={k1}: {int(written.sum())} of {written.size} written")
    arrs["cases_f"] = np.array([m[1] for m in meta], dtype=np.float32)
    arrs["cases_k1"] = np.array([m[2] for m in meta], dtype=np.float32)
    arrs["cases_image"] = np.array([m[0] for m in meta])
    np.savez_compressed(os.path.join(HERE, "g6_undistort.npz"), **arrs)
    print("wrote g6_undistort.npz,", os.path.getsize(os.path.join(HERE, "g6_undistort.npz")), "bytes")


if __name__ == "__main__":
    main()
