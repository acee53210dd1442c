// kernel_seed_tree.hip -- the octree the second half of Scene::initPatches builds from the surviving seeds (reference
// src/hpmvs/Scene.cpp:183-199: getBoundingBox, swapRoot, the scale floor, patchTree_.add per survivor), as sort / scan / sort
// (the arithmetic and the argument are in seed_tree.hpp, which the tests also compile for the host).
//
//   box      wave reduction of the centres' ordered integer images, one atomic per wavefront and axis
//   keys     per row: floored scale (written back), d(e), the 21-level path key          -> radix sort (key, row)
//   steps    per sorted position: the clamp of the step from its left and from its right -> one inclusive scan per side
//   depths   D = max(d, left(0), right(0)); leaf key = the D-level prefix, by row         -> radix sort (leaf key, row), stable:
//            leaves in Leaf_iterator order, rows in data order
//   heads    run heads                                                                   -> inclusive sum = leaf index + 1
//   emit     rows, cell_start, and per head the leaf's Cell by the reference's descent, its level and data[0]'s centre
//
// Everything is memory-bound and elementwise apart from the two sorts; the device block `blk` carries the box, the counts and a
// refusal flag (a root that is not finite) that every writing kernel honours, so the host reads one record back at the end.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "launch.h"
#include "seed_tree.hpp"

namespace hpmvs {

using seed::Clamp;

__device__ __forceinline__ seed::Root seed_root(const int32_t* blk, int maxlevel) {
    float mn[3], mx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mn[k] = seed::unordered((uint32_t)blk[kSeedBlkMin + k]);
        mx[k] = seed::unordered((uint32_t)blk[kSeedBlkMax + k]);
    }
    return seed::make_root(mn, mx, blk[kSeedBlkRows], maxlevel);
}

__global__ void seed_tree_init_kernel(int32_t* blk) {
    const int k = threadIdx.x;
    if (k >= kSeedBlkInts) return;
    int32_t v = 0;
    if (k >= kSeedBlkMin && k < kSeedBlkMin + 3) v = (int32_t)seed::ordered(FLT_MAX);
    if (k >= kSeedBlkMax && k < kSeedBlkMax + 3) v = (int32_t)seed::ordered(FLT_MIN);
    blk[k] = v;
}

__global__ void __launch_bounds__(256) seed_tree_box_kernel(const float* __restrict__ center, const uint8_t* __restrict__ ok, int n,
                                                            int32_t* blk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n && (!ok || ok[i]);
    uint32_t lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = seed::ordered(FLT_MAX);
        hi[k] = seed::ordered(FLT_MIN);
        if (in) {
            const float x = center[4 * (size_t)i + k];
            if (x == x) {   // std::min / std::max: a NaN never enters; below FLT_MAX / above FLT_MIN by the comparison itself
                const uint32_t o = seed::ordered(x);
                lo[k] = o < lo[k] ? o : lo[k];
                hi[k] = o > hi[k] ? o : hi[k];
            }
        }
    }
    const int count = __popcll(__ballot(in));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t a = __shfl_xor(lo[k], off), b = __shfl_xor(hi[k], off);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    if ((threadIdx.x & 63) == 0 && count > 0) {
        uint32_t* u = (uint32_t*)blk;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&u[kSeedBlkMin + k], lo[k]);
            atomicMax(&u[kSeedBlkMax + k], hi[k]);
        }
        atomicAdd(&blk[kSeedBlkRows], count);
    }
}

__global__ void __launch_bounds__(256) seed_tree_keys_kernel(const float* __restrict__ center, float* __restrict__ scale,
                                                             const uint8_t* __restrict__ ok, int n, int maxlevel, int32_t* blk,
                                                             unsigned long long* key, int32_t* row, int32_t* dep) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const seed::Root r = seed_root(blk, maxlevel);
    if (i == 0) {
        float* f = (float*)(blk + kSeedBlkInfo);
        f[0] = r.c[0]; f[1] = r.c[1]; f[2] = r.c[2]; f[3] = r.w; f[4] = r.floor;
        blk[kSeedBlkInfo + 5] = blk[kSeedBlkRows];
        blk[kSeedBlkBad] = r.finite ? 0 : 1;
    }
    if (i >= n || !r.finite) return;
    row[i] = i;
    if (ok && !ok[i]) {
        key[i] = seed::kAbsent;
        dep[i] = 0;
        return;
    }
    const float s = seed::floored(scale[i], r.floor);
    scale[i] = s;
    dep[i] = seed::depth_alone(r.w, s);
    const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
    key[i] = seed::path_key(r, p);
}

// sorted position i: left[i] the step from i - 1, right[n - 1 - i] the step from i + 1
__global__ void __launch_bounds__(256) seed_tree_steps_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ row,
                                                              const int32_t* __restrict__ dep, int n, const int32_t* __restrict__ blk,
                                                              Clamp* left, Clamp* right) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int n_rows = blk[kSeedBlkBad] ? 0 : blk[kSeedBlkRows];
    const bool prev = i > 0 && i < n_rows, next = i < n_rows - 1;
    const unsigned long long k = key[i];
    left[i] = seed::left_step(i, n_rows, prev ? seed::lcp(key[i - 1], k) : 0, prev ? dep[row[i - 1]] : 0);
    right[n - 1 - i] = seed::right_step(i, n_rows, next ? seed::lcp(k, key[i + 1]) : 0, next ? dep[row[i + 1]] : 0);
}

__global__ void __launch_bounds__(256) seed_tree_depths_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ row,
                                                               const int32_t* __restrict__ dep, const Clamp* __restrict__ left,
                                                               const Clamp* __restrict__ right, int n, const int32_t* __restrict__ blk,
                                                               unsigned long long* leaf_key, int32_t* depth) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || blk[kSeedBlkBad]) return;
    const int r = row[i];
    if (i >= blk[kSeedBlkRows]) {
        leaf_key[r] = seed::kAbsent;
        depth[r] = 0;
        return;
    }
    const int D = seed::final_depth(dep[r], left[i], right[n - 1 - i]);
    leaf_key[r] = seed::leaf_key(key[i], D);
    depth[r] = D;
}

__global__ void __launch_bounds__(256) seed_tree_heads_kernel(const unsigned long long* __restrict__ leaf_key, int n,
                                                              const int32_t* __restrict__ blk, int32_t* head) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int n_rows = blk[kSeedBlkBad] ? 0 : blk[kSeedBlkRows];
    head[j] = j < n_rows && (j == 0 || leaf_key[j] != leaf_key[j - 1]);
}

// entry j of every output: the run heads write their leaf (index pos - 1 < n_leaves), everything from n_rows / n_leaves on is 0
__global__ void __launch_bounds__(256) seed_tree_emit_kernel(SeedTreeOut o, const float* __restrict__ center, const int32_t* __restrict__ row,
                                                             const int32_t* __restrict__ depth, const int32_t* __restrict__ head,
                                                             const int32_t* __restrict__ pos, int n, int maxlevel, int32_t* blk) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || blk[kSeedBlkBad]) return;
    const int n_rows = blk[kSeedBlkRows];
    const int n_leaves = n_rows > 0 ? pos[n_rows - 1] : 0;
    if (j == 0) {
        blk[kSeedBlkInfo + 6] = n_leaves;
        o.cell_start[n_leaves] = n_rows;
    }
    o.rows[j] = j < n_rows ? row[j] : 0;
    if (j + 1 > n_leaves) o.cell_start[j + 1] = 0;
    if (j >= n_leaves) {
        o.cell_width[j] = 0.f;
        o.cell_level[j] = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o.cell_center[3 * (size_t)j + k] = 0.f;
            if (o.patch_center) o.patch_center[3 * (size_t)j + k] = 0.f;
        }
    }
    if (j >= n_rows || !head[j]) return;
    const int l = pos[j] - 1, r = row[j], D = depth[r];
    const float p[3] = {center[4 * (size_t)r], center[4 * (size_t)r + 1], center[4 * (size_t)r + 2]};
    const seed::Root root = seed_root(blk, maxlevel);
    float c[3], w;
    seed::descend(root, p, D, c, w);
    o.cell_start[l] = j;
    o.cell_width[l] = w;
    o.cell_level[l] = D;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.cell_center[3 * (size_t)l + k] = c[k];
        if (o.patch_center) o.patch_center[3 * (size_t)l + k] = p[k];
    }
}

size_t seed_tree_temp_bytes(int n) {
    size_t a = 0, b = 0, c = 0;
    const size_t m = (size_t)n;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const int32_t*)nullptr,
                                    (int32_t*)nullptr, m, 0u, 64u, (hipStream_t) nullptr);
    (void)rocprim::inclusive_scan(nullptr, b, (const Clamp*)nullptr, (Clamp*)nullptr, m, seed::ClampThen(), (hipStream_t) nullptr);
    (void)rocprim::inclusive_scan(nullptr, c, (const int32_t*)nullptr, (int32_t*)nullptr, m, rocprim::plus<int32_t>(), (hipStream_t) nullptr);
    a = a > b ? a : b;
    a = a > c ? a : c;
    return a ? a : 1;
}

int launch_seed_tree(const float* center, float* scale, const uint8_t* ok, int n, int maxlevel, const SeedTreeScratch& s,
                     const SeedTreeOut& out, hipStream_t st) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    size_t tb = s.temp_bytes;
    hipLaunchKernelGGL(seed_tree_init_kernel, dim3(1), dim3(64), 0, st, s.blk);
    hipLaunchKernelGGL(seed_tree_box_kernel, grid, block, 0, st, center, ok, n, s.blk);
    hipLaunchKernelGGL(seed_tree_keys_kernel, grid, block, 0, st, center, scale, ok, n, maxlevel, s.blk, s.key_a, s.row_a, s.dep);
    if (rocprim::radix_sort_pairs(s.temp, tb, (const unsigned long long*)s.key_a, s.key_b, (const int32_t*)s.row_a, s.row_b, (size_t)n, 0u, 64u,
                                  st) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(seed_tree_steps_kernel, grid, block, 0, st, s.key_b, s.row_b, s.dep, n, s.blk, s.pair_a, s.pair_b);
    tb = s.temp_bytes;
    if (rocprim::inclusive_scan(s.temp, tb, (const Clamp*)s.pair_a, s.pair_c, (size_t)n, seed::ClampThen(), st) != hipSuccess) return 1;
    tb = s.temp_bytes;
    if (rocprim::inclusive_scan(s.temp, tb, (const Clamp*)s.pair_b, s.pair_a, (size_t)n, seed::ClampThen(), st) != hipSuccess) return 1;
    // (key_a is free after the first sort: the leaf keys go there, by row; row_a still counts 0 .. n - 1)
    hipLaunchKernelGGL(seed_tree_depths_kernel, grid, block, 0, st, s.key_b, s.row_b, s.dep, s.pair_c, s.pair_a, n, s.blk, s.key_a, s.depth);
    tb = s.temp_bytes;
    if (rocprim::radix_sort_pairs(s.temp, tb, (const unsigned long long*)s.key_a, s.key_b, (const int32_t*)s.row_a, s.row_b, (size_t)n, 0u, 64u,
                                  st) != hipSuccess)
        return 1;
    int32_t* head = (int32_t*)s.pair_b;
    int32_t* pos = (int32_t*)s.pair_c;
    hipLaunchKernelGGL(seed_tree_heads_kernel, grid, block, 0, st, s.key_b, n, s.blk, head);
    tb = s.temp_bytes;
    if (rocprim::inclusive_scan(s.temp, tb, (const int32_t*)head, pos, (size_t)n, rocprim::plus<int32_t>(), st) != hipSuccess) return 1;
    hipLaunchKernelGGL(seed_tree_emit_kernel, grid, block, 0, st, out, center, s.row_b, s.depth, head, pos, n, maxlevel, s.blk);
    return 0;
}

}  // namespace hpmvs
