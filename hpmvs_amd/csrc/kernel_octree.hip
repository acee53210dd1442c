// kernel_octree.hip -- the leaf look-ups of CellProcessor::extend against the scheduler's real octree, for a whole level's points
// (include/hpmvs_amd.h: hpmvs_octree_locate_batch).  Every rule is octree.hpp's; this file only gives it lanes.
//
//   octree_build_kernel    one lane per key of either set: form check, then the key enters the open-addressing table with a
//                          compare-and-swap (finding itself there already is the "twice" verdict)
//   octree_check_kernel    one lane per key, against the finished table: the parent prefix is a branch or the root
//   octree_locate_kernel   one lane per point: up to 21 dependent table look-ups down the path, then contains / add_target in
//                          registers.  A point is 12 bytes in and 41 bytes out; the look-ups hit a table of 12 bytes per slot that
//                          stays in L2 for the trees of a scene (2 x (branches + leaves) slots), so the lanes need no cooperation:
//                          unlike regularize's 24 probes per cell there is one chain per item, and a level's 6 n points already
//                          give every SIMD its waves.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) octree_build_kernel(const unsigned long long* __restrict__ branch_key, int nb,
                                                           const unsigned long long* __restrict__ leaf_key, int nl,
                                                           unsigned long long* keys, int32_t* vals, uint32_t slots, int32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb + nl) return;
    const bool branch = i < nb;
    const unsigned long long key = branch ? branch_key[i] : leaf_key[i - nb];
    const int form = octree::key_form(key, branch);
    if (form) { atomicOr(verdict, form); return; }
    const unsigned long long mask = (unsigned long long)slots - 1;
    unsigned long long h = octree::hash(key) & mask;
    while (true) {   // slots >= 2 (nb + nl): a free slot exists
        const unsigned long long prev = atomicCAS(&keys[h], 0ull, key);
        if (prev == 0ull) { vals[h] = branch ? octree::kBranch : i - nb; return; }
        if (prev == key) { atomicOr(verdict, octree::kBadTwice); return; }
        h = (h + 1) & mask;
    }
}

__global__ void __launch_bounds__(256) octree_check_kernel(const unsigned long long* __restrict__ branch_key, int nb,
                                                           const unsigned long long* __restrict__ leaf_key, int nl, octree::Table t,
                                                           int32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb + nl) return;
    const unsigned long long key = i < nb ? branch_key[i] : leaf_key[i - nb];
    if (octree::key_form(key, i < nb)) return;   // (reported by the build kernel; its parent prefix means nothing)
    const int bad = octree::key_parentage(t, key);
    if (bad) atomicOr(verdict, bad);
}

__global__ void __launch_bounds__(256) octree_locate_kernel(octree::Cell root, octree::Table t, int n, const float* __restrict__ points,
                                                            const float* __restrict__ add_width, OctreeLocateOut out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    const octree::Located r = octree::locate(root, t, p);
    if (out.inside) out.inside[i] = octree::contains(root, p) ? 1 : 0;
    if (out.leaf_key) out.leaf_key[i] = r.key;
    if (out.leaf_index) out.leaf_index[i] = r.index;
    if (out.leaf_width) out.leaf_width[i] = r.cell.w;
    if (out.leaf_center) {
        out.leaf_center[3 * (size_t)i] = r.cell.c[0];
        out.leaf_center[3 * (size_t)i + 1] = r.cell.c[1];
        out.leaf_center[3 * (size_t)i + 2] = r.cell.c[2];
    }
    if (out.target_key) out.target_key[i] = add_width ? octree::add_target(r, p, add_width[i]) : 0ull;
}

void launch_octree_build(const unsigned long long* branch_key, int nb, const unsigned long long* leaf_key, int nl, unsigned long long* keys,
                         int32_t* vals, uint32_t slots, int32_t* verdict, hipStream_t st) {
    const int n = nb + nl;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(octree_build_kernel, grid, dim3(256), 0, st, branch_key, nb, leaf_key, nl, keys, vals, slots, verdict);
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    hipLaunchKernelGGL(octree_check_kernel, grid, dim3(256), 0, st, branch_key, nb, leaf_key, nl, t, verdict);
}

void launch_octree_locate(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n,
                          const float* points, const float* add_width, const OctreeLocateOut& out, hipStream_t st) {
    if (n <= 0) return;
    const octree::Cell r{{root[0], root[1], root[2]}, root[3]};
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    hipLaunchKernelGGL(octree_locate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r, t, n, points, add_width, out);
}

}  // namespace hpmvs
