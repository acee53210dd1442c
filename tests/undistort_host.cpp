// Host restatement of the level-0 undistortion (reference Image::undistort, src/hpmvs/Image.cpp:68-146): the
// product's map and sampling code (hpmvs_amd/csrc/undistort.hpp) compiled by g++ against glibc, the library the
// reference's float64 / std::complex<double> arithmetic runs on.  tests/test_cpu_undistort.py pins it to the
// reference's own output (tests/golden/g6_undistort.npz); the GPU tests and tools/undistort_scale.py compare the
// kernel with it.  Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared -pthread undistort_host.cpp
#include <cstdint>
#include <thread>
#include <vector>

#include "../hpmvs_amd/csrc/undistort.hpp"

using namespace hpmvs::ud;

static void rows(const uint8_t* src, int w, int h, float f, float k1, uint8_t* dst, uint8_t* written, int y0, int y1) {
    for (int iy = y0; iy < y1; iy++)
        for (int ix = 0; ix < w; ix++) {
            float sx, sy;
            const bool in = source_point(ix, iy, w, h, f, k1, &sx, &sy);
            const size_t o = (size_t)iy * w + ix;
            for (int c = 0; c < 3; c++) dst[3 * o + c] = in ? sample(src, w, h, sx, sy, c) : 0;
            if (written) written[o] = in;
        }
}

extern "C" {

// xy: [h][w][2] source point of every output pixel
void ud_map(int w, int h, float f, float k1, float* xy) {
    for (int iy = 0; iy < h; iy++)
        for (int ix = 0; ix < w; ix++) {
            const size_t o = (size_t)iy * w + ix;
            source_point(ix, iy, w, h, f, k1, &xy[2 * o], &xy[2 * o + 1]);
        }
}

// src, dst: interleaved u8 RGB [h][w][3]; written (may be null): [h][w], 1 where the reference writes the pixel.
// Unwritten pixels are 0.  `threads` > 1 splits the rows.
void ud_image(const uint8_t* src, int w, int h, float f, float k1, uint8_t* dst, uint8_t* written, int threads) {
    if (threads <= 1) {
        rows(src, w, h, f, k1, dst, written, 0, h);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(rows, src, w, h, f, k1, dst, written, (int)((long)h * t / threads), (int)((long)h * (t + 1) / threads));
    for (auto& th : pool) th.join();
}

}  // extern "C"
