#!/usr/bin/env python3
"""Generates tests/golden/g9_depth_vis.npz from the reference's vendored CImg: what Scene::visualizeDepths
(src/hpmvs/Scene.cpp:434-516) makes of a float image -- `if (v == MAX_DEPTH) v = 0`, normalize(0, 255.0),
map(CImg<unsigned char>::jet_LUT256()) -- and the 256-entry colormap itself.  The driver below is compiled in a temporary
directory against the reference's CImg.h (-Dcimg_display=0); data only is committed: the seeded input images, their RGB
results and the colormap.

    python tests/golden/make_golden_depth_vis.py [REFERENCE_ROOT]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_DEPTH = np.float32(1000.0)

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
using namespace cimg_library;
static const float MAX_DEPTH = 1000.0f;

// argv: cases.bin out.bin.  cases: per case int32 W, H, then W * H floats, pixel (x, y) at x + y * W.
// out: 768 bytes of the colormap, entry i at 3 i .. 3 i + 2, then per case W * H * 3 bytes, 3 * (y * W + x) + c.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    const CImg<unsigned char>& lut = CImg<unsigned char>::jet_LUT256();
    if (lut.width() != 1 || lut.height() != 256 || lut.depth() != 1 || lut.spectrum() != 3) return 4;
    for (int i = 0; i < 256; i++)
        for (int c = 0; c < 3; c++) fputc(lut(0, i, 0, c), fo);
    int32_t hd[2];
    while (fread(hd, 4, 2, fi) == 2) {
        const int W = hd[0], H = hd[1];
        std::vector<float> in((size_t)W * H);
        if (fread(in.data(), 4, in.size(), fi) != in.size()) return 5;
        CImg<float> img(W, H, 1, 1);
        for (int yy = 0; yy < img.height(); yy++)
            for (int xx = 0; xx < img.width(); xx++) {
                img._atXY(xx, yy) = in[(size_t)xx + (size_t)yy * W];
                if (img._atXY(xx, yy) == MAX_DEPTH) img._atXY(xx, yy) = 0;
            }
        img.normalize(0, 255.0);
        CImg<unsigned char> cmapImg = img.map(CImg<unsigned char>::jet_LUT256());
        for (int yy = 0; yy < H; yy++)
            for (int xx = 0; xx < W; xx++)
                for (int c = 0; c < 3; c++) fputc(cmapImg(xx, yy, 0, c), fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
"""


def depths(rng, h, w):
    """the scene's depths, 20 .. 45, in steps of 1 / 32 (few mantissa bits: the file stays small)"""
    return (rng.integers(20 * 32, 45 * 32 + 1, size=(h, w)) / 32.0).astype(np.float32)


def cases():
    """[(name, float32 [H, W])] in a fixed order; the shapes are those of the depth maps of the GPU test's views"""
    rng = np.random.default_rng(0x44565339)
    out = []
    out.append(("all_empty", np.full((23, 35), MAX_DEPTH, np.float32)))
    out.append(("one_depth", np.full((11, 17), 37.5, np.float32)))
    a = np.full((5, 8), MAX_DEPTH, np.float32)
    a[3, 6] = 12.25
    out.append(("one_cell", a))
    a = depths(rng, 23, 35)
    a[0, 0], a[-1, -1] = 19.5, 45.75      # the minimum in the first memory position, the maximum in the last
    out.append(("min_first_max_last", a))
    a = depths(rng, 11, 17)
    a[0, 0], a[-1, -1] = 45.75, 19.5
    out.append(("max_first_min_last", a))
    a = depths(rng, 5, 8) - np.float32(30.0)
    a[1, 2] = -7.125
    a[4, 0] = MAX_DEPTH
    out.append(("negative", a))
    # exactly 0 .. 255: normalize() leaves the image as it is and map() truncates
    a = (rng.integers(0, 255 * 16 + 1, size=(24, 32)) / 16.0).astype(np.float32)
    a[5, 7], a[20, 1], a[0, 31] = 0.0, 255.0, MAX_DEPTH
    a[3, 3], a[3, 4] = np.nextafter(np.float32(200.0), np.float32(0.0)), 200.0
    out.append(("range_0_255", a))
    # m = 0 (an empty cell), M = 510: v / 510 * 255 is exactly j for v = 2 j and just below j for the float below 2 j
    j = rng.integers(1, 255, size=(12, 16))
    a = (2.0 * j).astype(np.float32)
    below = rng.random(size=a.shape) < 0.5
    a[below] = np.nextafter(a[below], np.float32(0.0))
    a[0, 0], a[11, 15], a[6, 6] = MAX_DEPTH, 510.0, 2.0
    out.append(("on_and_below_integers", a))
    a = depths(rng, 48, 64)
    a[rng.random(size=a.shape) < 0.5] = MAX_DEPTH
    out.append(("sparse_64x48", a))
    out.append(("dense_35x23", depths(rng, 23, 35)))
    out.append(("one_by_one", np.full((1, 1), 30.0, np.float32)))
    a = depths(rng, 13, 1)
    a[4, 0] = MAX_DEPTH
    out.append(("one_by_n", a))
    a = depths(rng, 4, 5)
    a[rng.random(size=a.shape) < 0.3] = MAX_DEPTH
    out.append(("sparse_5x4", a))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
            fh.write(DRIVER)
        exe = os.path.join(tmp, "ref_depth_vis")
        cimg = os.path.join(ref, "thirdLibs", "cimg")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Dcimg_display=0", "-include", os.path.join(cimg, "CImg.h"),
                        os.path.join(tmp, "driver.cpp"), "-o", exe, "-lpthread"], check=True)
        fi, fo = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        with open(fi, "wb") as fh:
            for _, a in cs:
                fh.write(np.array([a.shape[1], a.shape[0]], np.int32).tobytes() + np.ascontiguousarray(a, np.float32).tobytes())
        subprocess.run([exe, fi, fo], check=True)
        raw = np.fromfile(fo, dtype=np.uint8)
    arrs = {"lut": raw[:768].reshape(256, 3).copy(), "names": np.array([n for n, _ in cs])}
    at = 768
    for n, a in cs:
        h, w = a.shape
        arrs[n + "_in"] = a
        arrs[n + "_rgb"] = raw[at:at + 3 * h * w].reshape(h, w, 3).copy()
        at += 3 * h * w
        print(f"{n}: {w}x{h}, {len(np.unique(arrs[n + '_rgb'].reshape(-1, 3), axis=0))} colours")
    assert at == raw.size
    path = os.path.join(HERE, "g9_depth_vis.npz")
    np.savez_compressed(path, **arrs)
    print("wrote g9_depth_vis.npz,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
