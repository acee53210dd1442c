// kernel_jpeg_encode.hip -- a level's interleaved RGB in HBM -> the entropy data of a baseline JPEG file (jpeg_enc.hpp;
// reference Scene::saveAsNVM through CImg's save_jpeg and libjpeg's defaults; restated in loops by tests/jpeg_enc_host.cpp).
//   jpeg_enc_coef_kernel     one wavefront per 16x16 MCU: colour conversion, edge replication, h2v2 downsampling, the
//                            "islow" forward DCT and the quantiser; the six blocks' int16 coefficients in zigzag order and
//                            scan order, dummy blocks filled.  The YCbCr samples live in LDS only.
//   jpeg_enc_length_kernel   per block: the DC predecessor by index arithmetic and the length of the block's code in bits
//   (rocPRIM exclusive scan, 64-bit: where every block's code starts)
//   jpeg_enc_write_kernel    per block: its code at its offset into the zero-filled stream (MSB first; the words two
//                            blocks share are OR-ed atomically), the last block pads the last byte with ones
//   jpeg_enc_ff_kernel       per 64-byte chunk of the stream: its 0xFF bytes   (scan: how far every chunk moves)
//   jpeg_enc_stuff_kernel    per chunk: its bytes at their final place, a 0x00 behind every 0xFF
// Every load and store is bounded by the array it goes to: the pixel addresses are clamped to the image, the block and
// chunk kernels return behind the last block / chunk, and a block's bits end where the scan says the next block starts.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "launch.h"

namespace hpmvs {

namespace {

constexpr int kTabWords = (int)(sizeof(jpge::EncTables) / 4);

__device__ void load_tables(const jpge::EncTables* __restrict__ g, uint32_t* s, int tid, int n) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(g);
    for (int k = tid; k < kTabWords; k += n) s[k] = w[k];
}

// LDS of one wavefront's MCU
struct McuTile {
    uint8_t y[16][16], cb[16][16], cr[16][16];
    uint8_t c[2][8][8];      // downsampled chroma
    int32_t ws[6][8][9];     // the DCT's work space: rows after pass 1, natural order after pass 2 (padded rows)
    int16_t out[6][64];      // quantised, zigzag order
};

}  // namespace

// 4 MCUs per workgroup, one per wavefront.  Lane l loads the four pixels (4 (l & 3) .., l >> 2) of the tile; lanes 0 .. 47
// run one row or one column of one block through fdct_1d; all lanes quantise and store (768 contiguous bytes per MCU).
__global__ void __launch_bounds__(256) jpeg_enc_coef_kernel(const uint8_t* __restrict__ rgb, jpge::Geom g, const jpge::EncTables* __restrict__ tabs,
                                                            int16_t* __restrict__ coef) {
    __shared__ McuTile tiles[4];
    __shared__ uint16_t s_q8[2][64];
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x, lane = tid & 63;
    McuTile& t = tiles[tid >> 6];
    if (tid < 128) s_q8[tid >> 6][tid & 63] = tabs->q8[tid >> 6][tid & 63];
    else if (tid < 192) s_zz[tid - 128] = tabs->zz[tid - 128];
    const uint32_t n_mcus = (uint32_t)g.mcux * (uint32_t)g.mcuy;
    const uint32_t m = blockIdx.x * 4u + (uint32_t)(tid >> 6);
    const bool live = m < n_mcus;
    const int my = live ? (int)(m / (uint32_t)g.mcux) : 0, mx = live ? (int)(m - (uint32_t)my * (uint32_t)g.mcux) : 0;
    {
        const int ty = lane >> 2, tx = 4 * (lane & 3);
        const int y = min(16 * my + ty, g.H - 1), x0 = 16 * mx + tx;
        const uint8_t* row = rgb + 3 * (size_t)y * (size_t)g.W;
        uint8_t px[12];
        const uint8_t* p = row + 3 * (size_t)x0;
        if (x0 + 3 < g.W && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t w = p4[k];
                px[4 * k] = (uint8_t)w; px[4 * k + 1] = (uint8_t)(w >> 8); px[4 * k + 2] = (uint8_t)(w >> 16); px[4 * k + 3] = (uint8_t)(w >> 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint8_t* q = row + 3 * (size_t)min(x0 + j, g.W - 1);
                px[3 * j] = q[0]; px[3 * j + 1] = q[1]; px[3 * j + 2] = q[2];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int yy, cb, cr;
            jpge::rgb_to_ycc(px[3 * j], px[3 * j + 1], px[3 * j + 2], &yy, &cb, &cr);
            t.y[ty][tx + j] = (uint8_t)yy; t.cb[ty][tx + j] = (uint8_t)cb; t.cr[ty][tx + j] = (uint8_t)cr;
        }
    }
    __syncthreads();
    {   // chroma sample (cx, cy): rows below the last one that holds image samples repeat that downsampled row
        const int cy = lane >> 3, cx = lane & 7;
        const int sy = min(8 * my + cy, g.ch - 1) - 8 * my;
        t.c[0][cy][cx] = (uint8_t)jpge::h2v2(t.cb[2 * sy][2 * cx], t.cb[2 * sy][2 * cx + 1], t.cb[2 * sy + 1][2 * cx], t.cb[2 * sy + 1][2 * cx + 1], cx);
        t.c[1][cy][cx] = (uint8_t)jpge::h2v2(t.cr[2 * sy][2 * cx], t.cr[2 * sy][2 * cx + 1], t.cr[2 * sy + 1][2 * cx], t.cr[2 * sy + 1][2 * cx + 1], cx);
    }
    __syncthreads();
    const int b = lane >> 3, r = lane & 7;  // (b < 6: lanes 0 .. 47)
    int32_t in[8], o[8];
    if (b < 6) {
#pragma unroll
        for (int k = 0; k < 8; k++) in[k] = (int32_t)(b < 4 ? t.y[8 * (b >> 1) + r][8 * (b & 1) + k] : t.c[b - 4][r][k]) - 128;
        jpge::fdct_1d(in, o, false);
#pragma unroll
        for (int k = 0; k < 8; k++) t.ws[b][r][k] = o[k];
    }
    __syncthreads();
    if (b < 6) {
#pragma unroll
        for (int k = 0; k < 8; k++) in[k] = t.ws[b][k][r];
        jpge::fdct_1d(in, o, true);
    }
    __syncthreads();
    if (b < 6) {
#pragma unroll
        for (int k = 0; k < 8; k++) t.ws[b][k][r] = o[k];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 6; j++) {  // block j, zigzag index `lane`
        const int nat = s_zz[lane];
        t.out[j][lane] = jpge::quantize(t.ws[j][nat >> 3][nat & 7], s_q8[j < 4 ? 0 : 1][lane]);
    }
    __syncthreads();
    if (!live) return;
    const int dummy = jpge::dummy_mask(g, mx, my);
    int16_t dc[4] = {t.out[0][0], t.out[1][0], t.out[2][0], t.out[3][0]};
    jpge::fill_dummy_dc(dc, dummy);
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + (size_t)m * 384);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int w = 64 * j + lane, blk = w >> 5, k = 2 * (w & 31);
        uint32_t v = (uint32_t)(uint16_t)t.out[blk][k] | (uint32_t)(uint16_t)t.out[blk][k + 1] << 16;
        if (blk < 4 && (dummy >> blk & 1)) v = k == 0 ? (uint32_t)(uint16_t)dc[blk] : 0u;
        dst[w] = v;
    }
}

// lens[b]: bits of block b's code; lens[n_blocks] stays 0, so that the exclusive scan ends with the total
__global__ void __launch_bounds__(256) jpeg_enc_length_kernel(const int16_t* __restrict__ coef, uint32_t n_blocks,
                                                              const jpge::EncTables* __restrict__ tabs, unsigned long long* __restrict__ lens) {
    __shared__ uint32_t s_tabs[kTabWords];
    load_tables(tabs, s_tabs, threadIdx.x, 256);
    __syncthreads();
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blocks) return;
    const long long p = jpge::dc_predecessor(b);
    jpge::LengthSink sink;
    jpge::encode_block(coef + (size_t)b * 64, p < 0 ? 0 : (int)coef[(size_t)p * 64], *reinterpret_cast<const jpge::EncTables*>(s_tabs),
                       b % 6u < 4u ? 0 : 1, sink);
    lens[b] = sink.bits;
}

namespace {

// A block's bits into the stream from bit `at` on, 32 at a time.  The first and the last word may hold a neighbour's bits
// and are OR-ed atomically into the zero-filled stream; the words between are this block's alone.  Bytes are in stream
// order, so a word is stored with its bytes swapped.
struct StreamSink {
    uint32_t* words;
    unsigned long long w;  // the word the next flush goes to
    unsigned long long acc = 0;  // bits not flushed yet, from bit 63 down
    int fill;  // of them, counting the neighbour's bits in front of the first word
    bool first = true;
    __device__ StreamSink(uint32_t* stream, unsigned long long at) : words(stream), w(at >> 5), fill((int)(at & 31)) {}
    __device__ void flush(bool whole) {
        const uint32_t v = __builtin_bswap32((uint32_t)(acc >> 32));
        if (first || !whole) atomicOr(&words[w], v);
        else words[w] = v;
        first = false;
    }
    __device__ void put(uint32_t code, int n) {  // n <= 16, so fill stays below 48
        if (n == 0) return;
        acc |= (unsigned long long)code << (64 - fill - n);
        fill += n;
        if (fill >= 32) {
            flush(true);
            acc <<= 32;
            fill -= 32;
            w++;
        }
    }
    __device__ void dc_category(int) {}
    __device__ void zrl() {}
    __device__ void finish() { if (fill > 0 && acc != 0) flush(false); }
};

}  // namespace

// offs: the exclusive scan of lens, n_blocks + 1 entries; stream: zero-filled, (offs[n_blocks] + 7) / 8 bytes rounded up to 64
__global__ void __launch_bounds__(256) jpeg_enc_write_kernel(const int16_t* __restrict__ coef, uint32_t n_blocks,
                                                             const jpge::EncTables* __restrict__ tabs, const unsigned long long* __restrict__ offs,
                                                             uint32_t* __restrict__ stream) {
    __shared__ uint32_t s_tabs[kTabWords];
    load_tables(tabs, s_tabs, threadIdx.x, 256);
    __syncthreads();
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blocks) return;
    const long long p = jpge::dc_predecessor(b);
    StreamSink sink(stream, offs[b]);
    jpge::encode_block(coef + (size_t)b * 64, p < 0 ? 0 : (int)coef[(size_t)p * 64], *reinterpret_cast<const jpge::EncTables*>(s_tabs),
                       b % 6u < 4u ? 0 : 1, sink);
    if (b + 1 == n_blocks) {  // the last byte is filled up with ones
        const int pad = (int)((8 - (offs[n_blocks] & 7)) & 7);
        sink.put((1u << pad) - 1u, pad);
    }
    sink.finish();
}

// cnt[c]: 0xFF bytes among the stream's bytes 64 c .. 64 c + 63 (the zero bytes behind the stream's end count nothing);
// cnt[n_chunks] stays 0
__global__ void __launch_bounds__(256) jpeg_enc_ff_kernel(const uint4* __restrict__ stream, unsigned long long n_chunks, unsigned long long* __restrict__ cnt) {
    const unsigned long long c = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (c >= n_chunks) return;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = stream[4 * c + k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
            n += ((w[j] & 0xffu) == 0xffu) + ((w[j] & 0xff00u) == 0xff00u) + ((w[j] & 0xff0000u) == 0xff0000u) + ((w[j] >> 24) == 0xffu);
    }
    cnt[c] = n;
}

// out: n_bytes + moved[n_chunks] bytes; chunk c's bytes start at 64 c + moved[c]
__global__ void __launch_bounds__(256) jpeg_enc_stuff_kernel(const uint4* __restrict__ stream, unsigned long long n_chunks, unsigned long long n_bytes,
                                                             const unsigned long long* __restrict__ moved, uint8_t* __restrict__ out) {
    const unsigned long long c = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (c >= n_chunks) return;
    const unsigned long long left = n_bytes - 64 * c;
    const int n = left < 64 ? (int)left : 64;
    uint8_t* o = out + 64 * c + moved[c];
    uint8_t* const end = out + 64 * c + n + moved[c + 1];  // where the next chunk's bytes start, or the output ends
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = stream[4 * c + k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint8_t byte = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            if (16 * k + j < n && o < end) {
                *o++ = byte;
                if (byte == 0xff && o < end) *o++ = 0;
            }
        }
    }
}

void launch_jpeg_enc_coef(const uint8_t* rgb, const jpge::Geom& g, const jpge::EncTables* tabs, int16_t* coef, hipStream_t st) {
    const uint32_t n_mcus = (uint32_t)g.mcux * (uint32_t)g.mcuy;
    hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3((n_mcus + 3) / 4), dim3(256), 0, st, rgb, g, tabs, coef);
}
void launch_jpeg_enc_lengths(const int16_t* coef, uint32_t n_blocks, const jpge::EncTables* tabs, unsigned long long* lens, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_enc_length_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, st, coef, n_blocks, tabs, lens);
}
int jpeg_enc_scan(void* temp, size_t* temp_bytes, const unsigned long long* in, unsigned long long* out, size_t n, hipStream_t st) {
    return (int)rocprim::exclusive_scan(temp, *temp_bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), st);
}
void launch_jpeg_enc_write(const int16_t* coef, uint32_t n_blocks, const jpge::EncTables* tabs, const unsigned long long* offs, uint32_t* stream,
                           hipStream_t st) {
    hipLaunchKernelGGL(jpeg_enc_write_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, st, coef, n_blocks, tabs, offs, stream);
}
void launch_jpeg_enc_ff(const uint8_t* stream, unsigned long long n_chunks, unsigned long long* cnt, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_enc_ff_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(stream), n_chunks, cnt);
}
void launch_jpeg_enc_stuff(const uint8_t* stream, unsigned long long n_chunks, unsigned long long n_bytes, const unsigned long long* moved, uint8_t* out,
                           hipStream_t st) {
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(stream), n_chunks,
                       n_bytes, moved, out);
}

}  // namespace hpmvs
