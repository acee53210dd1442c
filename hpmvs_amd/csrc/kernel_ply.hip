// kernel_ply.hip -- the patch cloud as the file the reference's DynOctTree::toExtPly writes (include/hpmvs/doctree.h:526-622), made
// in HBM; the bytes are ply_text.hpp's, shared with the host restatement of the tests.  The file's body has two sections, all
// vertex lines (records) and then all visibility lines (lists); row r of the file is patch order[r], or patch r.
//
// ply_len_kernel: one lane per row.  ASCII: converts the row's seven floats ONCE into their digit records and the three colours
//   into their bytes, stores the ten words in scratch (rec[k][row]) and writes the length of the row's vertex line and of its
//   visibility line; binary: the fixed record length and 4 + 4 n.  The lowest row whose order entry is outside [0, n), or whose
//   n_images is outside [0, max_images], ends up in one error word (2 row + kind, by atomicMin).
// One exclusive 64-bit scan over [vertex lengths | list lengths | 0] gives every line its place: the list section starts where
//   the vertex section ends, and the last entry is the body's length.
// ply_vertex_kernel: a wavefront owns 64 consecutive rows, whose lines are contiguous in the file.  Every lane expands its row
//   into LDS at (its file offset - the block's file offset + the block's misalignment), so that the LDS copy and the file agree
//   modulo 16; then the whole wavefront copies the block: 16-byte stores over the aligned middle, byte stores on the ragged
//   head and tail.  No lane writes its line to global memory.
// ply_list_kernel: one wavefront per row, lanes strided over the ids; a wave prefix sum of the ids' text lengths (__shfl_up)
//   gives each lane the place of its id.  The binary list is written the same way with fixed lengths.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ply_text.hpp"

namespace hpmvs {

namespace {

constexpr int kThreads = 256;                  // four wavefronts
constexpr int kWaves = kThreads / 64;
constexpr int kWaveBytes = (64 * ply::kMaxVertexLine + 15 + 15) & ~15;   // a block of 64 lines behind up to 15 bytes of misalignment
static_assert(ply::kMaxVertexRecord <= ply::kMaxVertexLine, "a binary record fits a line's room");

__device__ __forceinline__ uint32_t bits_of(float v) { return __float_as_uint(v); }

}  // namespace

__global__ void __launch_bounds__(kThreads) ply_len_kernel(PlyRows A) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= A.n_rows) return;
    const size_t R = (size_t)A.n_rows;
    const int p = A.order ? A.order[r] : r;
    if (p < 0 || p >= A.n) {
        atomicMin(A.err, 2u * (unsigned)r);
        A.len[r] = 0ull; A.len[R + r] = 0ull;
        return;
    }
    unsigned long long vlen, llen = 0ull;
    if (A.flags & ply::kBinary) {
        vlen = (unsigned long long)ply::vertex_record_len(A.flags);
    } else {
        uint32_t* rec = A.rec + r;
        for (int k = 0; k < 3; k++) rec[k * R] = ply::float_record(bits_of(A.center[4 * (size_t)p + k]));
        if (A.flags & ply::kNormal)
            for (int k = 0; k < 3; k++) rec[(3 + k) * R] = ply::float_record(bits_of(A.normal[4 * (size_t)p + k]));
        for (int k = 0; k < 3; k++) rec[(6 + k) * R] = ply::colour_byte(bits_of(A.color[3 * (size_t)p + k]));
        if (A.flags & ply::kScale) rec[9 * R] = ply::float_record(bits_of(A.scale[p]));
        vlen = (unsigned long long)ply::vertex_line_len(rec, R, A.flags);
    }
    if (A.flags & ply::kVisibility) {
        int n = A.n_images[p];
        if (n < 0 || n > A.max_images) { atomicMin(A.err, 2u * (unsigned)r + 1u); n = 0; }
        llen = (A.flags & ply::kBinary) ? (unsigned long long)ply::list_record_len(n)
                                        : (unsigned long long)ply::list_line_len(n, A.images + (size_t)p * (size_t)A.max_images);
    }
    A.len[r] = vlen;
    A.len[R + r] = llen;
}

// body: the file behind its header; offs: the scan of len
__global__ void __launch_bounds__(kThreads) ply_vertex_kernel(PlyRows A, const unsigned long long* __restrict__ offs, uint8_t* __restrict__ body) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[kWaves][kWaveBytes];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = ((long long)blockIdx.x * kWaves + wave) * 64;   // the wavefront's first row
    const bool live = row0 < A.n_rows;                                     // (the same in all of its lanes)
    uint8_t* s = s_text[wave];
    unsigned long long block_at = 0ull, block_len = 0ull;
    unsigned a = 0u;
    if (live) {
        const long long last = row0 + 64 < A.n_rows ? row0 + 64 : A.n_rows;
        block_at = offs[row0];
        block_len = offs[last] - block_at;   // (offs[n_rows] is where the list section starts)
        a = (unsigned)((uintptr_t)(body + block_at) & 15u);
        const long long r = row0 + lane;
        if (r < A.n_rows) {
            uint8_t* mine = s + a + (size_t)(offs[r] - block_at);
            if (A.flags & ply::kBinary) {
                const size_t p = (size_t)(A.order ? A.order[r] : (int)r);
                uint32_t xyz[3], nrm[3] = {0u, 0u, 0u}, col[3];
                for (int k = 0; k < 3; k++) { xyz[k] = bits_of(A.center[4 * p + k]); col[k] = bits_of(A.color[3 * p + k]); }
                if (A.flags & ply::kNormal)
                    for (int k = 0; k < 3; k++) nrm[k] = bits_of(A.normal[4 * p + k]);
                ply::put_vertex_record(xyz, nrm, col, (A.flags & ply::kScale) ? bits_of(A.scale[p]) : 0u, A.flags, mine);
            } else {
                ply::put_vertex_line(A.rec + r, (size_t)A.n_rows, A.flags, mine);
            }
        }
    }
    __syncthreads();
    if (!live || block_len == 0ull) return;
    // [a, a + block_len) of s goes to the same offsets of g, which is 16-byte aligned
    uint8_t* g = body + block_at - a;
    const size_t begin = a, end = a + (size_t)block_len;
    const size_t mid0 = (begin + 15) & ~(size_t)15, mid1 = end & ~(size_t)15;
    if (mid0 >= mid1) {   // no whole 16 bytes
        for (size_t i = begin + lane; i < end; i += 64) g[i] = s[i];
        return;
    }
    if (begin + lane < mid0) g[begin + lane] = s[begin + lane];
    for (size_t i = mid0 + 16 * (size_t)lane; i < mid1; i += 16 * 64) *(uint4*)(g + i) = *(const uint4*)(s + i);
    if (mid1 + lane < end) g[mid1 + lane] = s[mid1 + lane];
}

__global__ void __launch_bounds__(kThreads) ply_list_kernel(PlyRows A, const unsigned long long* __restrict__ offs, uint8_t* __restrict__ body) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= A.n_rows) return;
    const size_t p = (size_t)(A.order ? A.order[r] : (int)r);
    const int n = A.n_images[p];
    const int32_t* ids = A.images + p * (size_t)A.max_images;
    uint8_t* o = body + offs[(size_t)A.n_rows + r];
    if (A.flags & ply::kBinary) {
        if (lane == 0) ply::put_le32((uint32_t)n, o);
        for (int k = lane; k < n; k += 64) ply::put_le32((uint32_t)ids[k], o + 4 + 4 * (size_t)k);
        return;
    }
    size_t base = (size_t)ply::uint_len((uint32_t)n) + 1;
    if (lane == 0) { ply::put_uint((uint32_t)n, o); o[base - 1] = ' '; }
    for (int k0 = 0; k0 < n; k0 += 64) {   // (n is the same in all lanes: every lane takes every turn)
        const int k = k0 + lane;
        const uint32_t id = k < n ? (uint32_t)ids[k] : 0u;
        const int len = k < n ? ply::uint_len(id) + 1 : 0;
        int incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (k < n) {
            uint8_t* mine = o + base + (size_t)(incl - len);
            ply::put_uint(id, mine);
            mine[len - 1] = ' ';
        }
        base += (size_t)__shfl(incl, 63);
    }
    if (lane == 0) o[base] = '\n';
}

void launch_ply_len(const PlyRows& A, hipStream_t st) {
    if (A.n_rows <= 0) return;
    hipLaunchKernelGGL(ply_len_kernel, dim3((unsigned)(((size_t)A.n_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, A);
}

void launch_ply_vertex(const PlyRows& A, const unsigned long long* offs, uint8_t* body, hipStream_t st) {
    if (A.n_rows <= 0) return;
    const size_t per = (size_t)kWaves * 64;
    hipLaunchKernelGGL(ply_vertex_kernel, dim3((unsigned)(((size_t)A.n_rows + per - 1) / per)), dim3(kThreads), 0, st, A, offs, body);
}

void launch_ply_list(const PlyRows& A, const unsigned long long* offs, uint8_t* body, hipStream_t st) {
    if (A.n_rows <= 0 || !(A.flags & ply::kVisibility)) return;
    hipLaunchKernelGGL(ply_list_kernel, dim3((unsigned)(((size_t)A.n_rows + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, A, offs, body);
}

}  // namespace hpmvs
