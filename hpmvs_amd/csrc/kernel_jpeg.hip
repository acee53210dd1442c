// kernel_jpeg.hip -- everything of a baseline JPEG decode behind the entropy decoder (jpeg.hpp; reference Image::load
// through CImg and libjpeg's defaults): jpeg_idct_kernel dequantises the host's int16 coefficient blocks, runs libjpeg's
// integer "islow" IDCT and writes one u8 sample plane per component; jpeg_rgb_kernel interpolates subsampled chroma
// (fancy h2v1 / h2v2), converts YCbCr and writes the interleaved u8 RGB level 0 the scene, launch_undistort and the
// pyramid kernel use.  Both move a few bytes per pixel and are bound by HBM traffic.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace hpmvs {

// 8 lanes per 8x8 block, 8 blocks per wavefront, 32 per workgroup.  Lane r of a block loads coefficient row r (16 bytes:
// the wavefront reads 1 KiB contiguous), the block is transposed through a padded LDS tile so that the column pass runs
// with lane = column, transposed back, and the row pass runs with lane = row: each lane ends with the 8 samples of one
// output row and stores them at once.  Columns first: the two passes round differently.
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const uint16_t* __restrict__ q, const int16_t* __restrict__ coef,
                                                        JpegBlocks B, jpg::Planes P, uint8_t* __restrict__ planes) {
    __shared__ uint16_t sq[3 * 64];
    __shared__ int32_t tile[32][8][9];
    const int tid = threadIdx.x;
    if (tid < 3 * 64) sq[tid] = q[tid];
    const int g = tid >> 3, r = tid & 7;
    const uint32_t blk = blockIdx.x * 32u + (uint32_t)g;
    const bool live = blk < B.n_blocks;
    const int comp = blk >= B.first2 ? 2 : blk >= B.first1 ? 1 : 0;
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (live) raw = *reinterpret_cast<const uint4*>(coef + (size_t)blk * 64 + r * 8);
    __syncthreads();
    const uint16_t* qr = sq + comp * 64 + r * 8;
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        tile[g][r][2 * j] = jpg::dequant((int16_t)(w[j] & 0xffffu), qr[2 * j]);
        tile[g][r][2 * j + 1] = jpg::dequant((int16_t)(w[j] >> 16), qr[2 * j + 1]);
    }
    __syncthreads();
    int32_t in[8], ws[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = tile[g][k][r];
    jpg::idct_1d(in, ws, jpg::kPass1Shift);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) tile[g][k][r] = ws[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = tile[g][r][k];
    jpg::idct_1d(in, ws, jpg::kPass2Shift);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo |= (uint32_t)jpg::range_limit(ws[k]) << (8 * k);
        hi |= (uint32_t)jpg::range_limit(ws[4 + k]) << (8 * k);
    }
    if (!live) return;
    const uint32_t first = comp == 2 ? B.first2 : comp == 1 ? B.first1 : 0u;
    const uint32_t bx = (uint32_t)(comp == 0 ? B.bx0 : B.bx12);
    const uint32_t off = comp == 2 ? P.off[2] : comp == 1 ? P.off[1] : P.off[0];
    const uint32_t local = blk - first, by = local / bx, cx = local - by * bx;
    *reinterpret_cast<uint2*>(planes + off + ((size_t)by * 8 + r) * (bx * 8) + cx * 8) = make_uint2(lo, hi);
}

// four horizontally adjacent output pixels (12 bytes) per work-item: three dword stores where the address allows it
__global__ void __launch_bounds__(256) jpeg_rgb_kernel(const uint8_t* __restrict__ planes, jpg::Planes P, uint8_t* __restrict__ rgb) {
    const int x0 = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int y = blockIdx.y;
    if (x0 >= P.W || y >= P.H) return;
    uint8_t px[12];
    jpg::convert_quad(planes, P, x0, y, px);
    uint8_t* o = rgb + 3 * ((size_t)y * P.W + x0);
    const int nb = 3 * (P.W - x0 < 4 ? P.W - x0 : 4);
    if (nb == 12 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; k++)
            o4[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (k < nb) o[k] = px[k];
    }
}

void launch_jpeg_idct(const uint16_t* q, const int16_t* coef, const JpegBlocks& B, const jpg::Planes& P, uint8_t* planes, hipStream_t st) {
    if (B.n_blocks == 0) return;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((B.n_blocks + 31) / 32), dim3(256), 0, st, q, coef, B, P, planes);
}

void launch_jpeg_rgb(const uint8_t* planes, const jpg::Planes& P, uint8_t* rgb, hipStream_t st) {
    if (P.W <= 0 || P.H <= 0) return;
    const unsigned quads = (unsigned)(P.W + 3) / 4;
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((quads + 255) / 256, P.H), dim3(256), 0, st, planes, P, rgb);
}

}  // namespace hpmvs
