// kernel_undistort.hip -- level-0 radial undistortion of a view (reference Image::undistort, src/hpmvs/Image.cpp:68-146):
// one work-item per output pixel computes the source point (undistort.hpp: float64, and std::complex<double> for
// k1 < 0, in the reference's operation order), samples the raw interleaved u8 level 0 bilinearly as CImg does and writes
// the truncated u8 result.  Pixels the reference never writes get 0.  Float64-issue bound: a few loads per pixel.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "undistort.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) undistort_kernel(const uint8_t* __restrict__ src, int w, int h, float f, float k1,
                                                        uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= w || iy >= h) return;
    float sx, sy;
    const bool in = ud::source_point(ix, iy, w, h, f, k1, &sx, &sy);
    uint8_t* o = dst + 3 * ((size_t)iy * w + ix);
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = in ? ud::sample(src, w, h, sx, sy, c) : 0;
}

__global__ void __launch_bounds__(256) undistort_map_kernel(int w, int h, float f, float k1, float* __restrict__ xy) {
#pragma clang fp contract(off)
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= w || iy >= h) return;
    float sx, sy;
    ud::source_point(ix, iy, w, h, f, k1, &sx, &sy);
    const size_t o = (size_t)iy * w + ix;
    xy[2 * o] = sx;
    xy[2 * o + 1] = sy;
}

void launch_undistort(const uint8_t* src, int w, int h, float f, float k1, uint8_t* dst, hipStream_t st) {
    if (w <= 0 || h <= 0) return;
    dim3 block(256), grid((w + 255) / 256, h);
    hipLaunchKernelGGL(undistort_kernel, grid, block, 0, st, src, w, h, f, k1, dst);
}

void launch_undistort_map(int w, int h, float f, float k1, float* xy, hipStream_t st) {
    if (w <= 0 || h <= 0) return;
    dim3 block(256), grid((w + 255) / 256, h);
    hipLaunchKernelGGL(undistort_map_kernel, grid, block, 0, st, w, h, f, k1, xy);
}

}  // namespace hpmvs
