// kernel_depth_vis.hip -- a view's depth maps as jet-coloured RGB images in HBM (reference Scene::visualizeDepths,
// src/hpmvs/Scene.cpp:434-516; the arithmetic is depth_vis.hpp's, shared with the host restatement of the tests).
//
// depth_vis_gather_kernel: the image's float values -- one level's cells, or the minimum over the levels for the combined image,
//   0 for an empty cell -- from the column-major maps (element (y, x) at y + x * rows) into a row-major scratch image (pixel
//   (x, y) at y * W + x), through a 64 x 64 LDS tile so that the reads run along y and the writes along x, both coalesced; the
//   tile's rows are padded by one dword, which keeps the transposed reads off each other's banks.  Every workgroup leaves the
//   least and the largest of its values: lanes by __shfl_xor, the four wavefronts through LDS.
// depth_vis_colour_kernel: every workgroup reduces the partials again (a few hundred pairs; a minimum and a maximum do not
//   depend on the order), then normalises, looks the colormap up in LDS and writes interleaved u8 RGB, 3 * (y * W + x) + c, the
//   layout jpeg_encode_device reads.
// Both are bandwidth-trivial: 12 bytes of traffic per pixel, 2 M pixels for a 3840 x 2160 view's level 0.
#include <hip/hip_runtime.h>

#include "depth_vis.hpp"
#include "launch.h"

namespace hpmvs {

namespace {

constexpr int kTile = 64;           // cells per tile side = lanes of a wavefront
constexpr int kThreads = 256;       // four wavefronts, 16 tile rows each
constexpr unsigned kColourBlocks = 2048;  // at most; a workgroup strides over the pixels beyond

// least and largest over a workgroup of kThreads; the result is valid in every thread
__device__ __forceinline__ void block_min_max(float& mn, float& mx, float (*s_red)[kThreads / 64]) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[0][wave] = mn; s_red[1][wave] = mx; }
    __syncthreads();
    mn = s_red[0][0]; mx = s_red[1][0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; w++) {
        mn = s_red[0][w] < mn ? s_red[0][w] : mn;
        mx = s_red[1][w] > mx ? s_red[1][w] : mx;
    }
}

}  // namespace

// level >= 0: that level's map; level < 0: the combined image over n_levels levels.  W x H: the image (cols x rows of the level,
// of level 0 for the combined image).  vals [H][W]; part [2][gridDim.x * gridDim.y]: the workgroups' minima, then their maxima.
__global__ void __launch_bounds__(kThreads) depth_vis_gather_kernel(DevDepthView D, int n_levels, int level, int W, int H,
                                                                    float* __restrict__ vals, float* __restrict__ part) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float s_red[2][kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    float mn = INFINITY, mx = -INFINITY;
    const int y = y0 + lane;
    for (int xl = wave; xl < kTile; xl += kThreads / 64) {
        const int x = x0 + xl;
        if (x < W && y < H) {
            const float d = level >= 0 ? D.d[level][(size_t)y + (size_t)x * (size_t)H]
                                       : dvis::combined_depth(D.d, D.rows, D.cols, n_levels, x, y);
            const float v = dvis::cell_value(d);
            tile[xl][lane] = v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
    }
    __syncthreads();
    const int x = x0 + lane;
    for (int yl = wave; yl < kTile; yl += kThreads / 64) {
        const int yy = y0 + yl;
        if (x < W && yy < H) vals[(size_t)yy * W + x] = tile[lane][yl];
    }
    block_min_max(mn, mx, s_red);   // (every workgroup holds a cell of the image, so both are finite)
    if (threadIdx.x == 0) {
        const unsigned b = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.x * gridDim.y;
        part[b] = mn;
        part[nb + b] = mx;
    }
}

// vals [n] -> rgb [n][3]; part [2][n_part] as depth_vis_gather_kernel left it; lut: the 768 bytes of dvis::make_colormap;
// range [2]: m and M as used, written by the first workgroup.
__global__ void __launch_bounds__(kThreads) depth_vis_colour_kernel(const float* __restrict__ vals, size_t n, const float* __restrict__ part,
                                                                    unsigned n_part, const uint8_t* __restrict__ lut, uint8_t* __restrict__ rgb,
                                                                    float* __restrict__ range) {
    __shared__ uint8_t s_lut[768];
    __shared__ float s_red[2][kThreads / 64];
    for (int k = threadIdx.x; k < 768; k += kThreads) s_lut[k] = lut[k];
    float m = INFINITY, M = -INFINITY;
    for (unsigned k = threadIdx.x; k < n_part; k += kThreads) {
        const float a = part[k], b = part[n_part + k];
        m = a < m ? a : m;
        M = b > M ? b : M;
    }
    block_min_max(m, M, s_red);
    __syncthreads();   // (s_lut; block_min_max's barrier lies before its last reads only)
    if (blockIdx.x == 0 && threadIdx.x == 0) { range[0] = m; range[1] = M; }
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const int idx = dvis::lut_index(vals[i], m, M);
        uint8_t* o = rgb + 3 * i;
        o[0] = s_lut[3 * idx]; o[1] = s_lut[3 * idx + 1]; o[2] = s_lut[3 * idx + 2];
    }
}

unsigned depth_vis_partials(int W, int H) { return (unsigned)((W + kTile - 1) / kTile) * (unsigned)((H + kTile - 1) / kTile); }

void launch_depth_vis_gather(const DevDepthView& D, int n_levels, int level, int W, int H, float* vals, float* part, hipStream_t st) {
    if (W <= 0 || H <= 0) return;
    dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile);
    hipLaunchKernelGGL(depth_vis_gather_kernel, grid, dim3(kThreads), 0, st, D, n_levels, level, W, H, vals, part);
}

void launch_depth_vis_colour(const float* vals, size_t n, const float* part, unsigned n_part, const uint8_t* lut, uint8_t* rgb, float* range,
                             hipStream_t st) {
    if (!n) return;
    size_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > kColourBlocks) blocks = kColourBlocks;
    hipLaunchKernelGGL(depth_vis_colour_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, vals, n, part, n_part, lut, rgb, range);
}

}  // namespace hpmvs
