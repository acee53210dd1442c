// kernel_extend_forest.hip -- one extend level's tree look-ups for ALL subtrees of a partition inside ONE expansion call
// (include/hpmvs_amd.h: hpmvs_extend_forest_batch).  Every rule is octree.hpp's; this file only gives it lanes.
//
//   forest_build_kernel         one lane per key of the whole forest: the owning tree by a binary search of the offsets, form
//                               check, then the key enters ITS TREE's slot range of the one table buffer with a compare-and-swap
//   forest_check_kernel         one lane per key, against the finished tables: the parent prefix is a branch or the root
//   forest_parents_kernel       one lane per parent: parent_tree[i] names a tree, and that tree has the level (a host byte)
//   extend_forest_pre_kernel    the body of extend_tree_pre_kernel, root and table read from trees[parent_tree[i / 6]]
//   extend_forest_post_kernel   the body of extend_tree_post_kernel, likewise
// The verdict is three words folded with atomicMin (the lowest offending tree first), read back once by the host.  A Tree is 40
// bytes; a level's few hundred of them stay in L2 beside the tables, so a candidate lane pays two more loads than a lone tree's.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) forest_build_kernel(int n_trees, const int32_t* __restrict__ branch_first,
                                                           const int32_t* __restrict__ leaf_first,
                                                           const unsigned long long* __restrict__ branch_key,
                                                           const unsigned long long* __restrict__ leaf_key, int n,
                                                           const octree::Tree* __restrict__ trees, uint32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const octree::ForestKey k = octree::forest_key(n_trees, branch_first, leaf_first, (const uint64_t*)branch_key, (const uint64_t*)leaf_key, i);
    const int form = octree::key_form(k.key, k.index == octree::kBranch);
    if (form) { atomicMin(&verdict[kForestTable], octree::forest_finding(k.tree, form)); return; }
    const octree::Table t = trees[k.tree].t;
    unsigned long long* keys = (unsigned long long*)t.keys;   // (the buffer is the call's own; Table is the readers' view of it)
    int32_t* vals = (int32_t*)t.vals;
    const unsigned long long mask = (unsigned long long)t.slots - 1;
    unsigned long long h = octree::hash(k.key) & mask;
    while (true) {   // slots >= 2 x the tree's keys: a free slot exists
        const unsigned long long prev = atomicCAS(&keys[h], 0ull, (unsigned long long)k.key);
        if (prev == 0ull) { vals[h] = k.index; return; }
        if (prev == k.key) { atomicMin(&verdict[kForestTable], octree::forest_finding(k.tree, octree::kBadTwice)); return; }
        h = (h + 1) & mask;
    }
}

__global__ void __launch_bounds__(256) forest_check_kernel(int n_trees, const int32_t* __restrict__ branch_first,
                                                           const int32_t* __restrict__ leaf_first,
                                                           const unsigned long long* __restrict__ branch_key,
                                                           const unsigned long long* __restrict__ leaf_key, int n,
                                                           const octree::Tree* __restrict__ trees, uint32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = octree::forest_check_key(
        trees, octree::forest_key(n_trees, branch_first, leaf_first, (const uint64_t*)branch_key, (const uint64_t*)leaf_key, i));
    if (v != octree::kForestGood) atomicMin(&verdict[kForestTable], v);
}

__global__ void __launch_bounds__(256) forest_parents_kernel(int n_trees, const uint8_t* __restrict__ has_level, int n,
                                                             const int32_t* __restrict__ parent_tree, uint32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k = parent_tree[i];
    if (k < 0 || k >= n_trees) atomicMin(&verdict[kForestParent], (uint32_t)i);
    else if (!has_level[k]) atomicMin(&verdict[kForestLevel], (uint32_t)k);
}

__global__ void __launch_bounds__(256) extend_forest_pre_kernel(const octree::Tree* __restrict__ trees,
                                                                const int32_t* __restrict__ parent_tree, int n, float width,
                                                                float add_width, const float* __restrict__ center,
                                                                int32_t* __restrict__ n_images, ExtendTreeOut out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
    const octree::ExtendPre r = octree::extend_forest_pre(trees, parent_tree[i / 6], p, width, add_width);
    if (out.skip) out.skip[i] = r.skip ? 1 : 0;
    if (out.pre_inside) out.pre_inside[i] = r.inside ? 1 : 0;
    if (out.pre_key) out.pre_key[i] = r.pre_key;
    if (r.skip && n_images[i] > 0) n_images[i] = -20;
}

__global__ void __launch_bounds__(256) extend_forest_post_kernel(const octree::Tree* __restrict__ trees,
                                                                 const int32_t* __restrict__ parent_tree, int n, float add_width,
                                                                 const float* __restrict__ center, const uint8_t* __restrict__ ok,
                                                                 ExtendTreeOut out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    octree::ExtendPost r{false, 0};
    if (ok[i]) {
        const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
        r = octree::extend_forest_post(trees, parent_tree[i / 6], p, add_width);
    }
    if (out.border) out.border[i] = r.border ? 1 : 0;
    if (out.post_key) out.post_key[i] = r.post_key;
}

void launch_forest_build(int n_trees, const int32_t* branch_first, const int32_t* leaf_first, const unsigned long long* branch_key,
                         const unsigned long long* leaf_key, int n_keys, const octree::Tree* trees, uint32_t* verdict, hipStream_t st) {
    if (n_keys <= 0) return;
    const dim3 grid((unsigned)((n_keys + 255) / 256));
    hipLaunchKernelGGL(forest_build_kernel, grid, dim3(256), 0, st, n_trees, branch_first, leaf_first, branch_key, leaf_key, n_keys, trees,
                       verdict);
    hipLaunchKernelGGL(forest_check_kernel, grid, dim3(256), 0, st, n_trees, branch_first, leaf_first, branch_key, leaf_key, n_keys, trees,
                       verdict);
}

void launch_forest_parents(int n_trees, const uint8_t* has_level, int n, const int32_t* parent_tree, uint32_t* verdict, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(forest_parents_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n_trees, has_level, n, parent_tree,
                       verdict);
}

void launch_extend_forest_pre(const octree::Tree* trees, const int32_t* parent_tree, int n, float width, const DevBatch& out,
                              const ExtendTreeOut& k, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(extend_forest_pre_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trees, parent_tree, n, width,
                       octree::extend_add_width(width), out.center, out.n_images, k);
}

void launch_extend_forest_post(const octree::Tree* trees, const int32_t* parent_tree, int n, float width, const DevBatch& out,
                               const ExtendTreeOut& k, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(extend_forest_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trees, parent_tree, n,
                       octree::extend_add_width(width), out.center, out.ok, k);
}

}  // namespace hpmvs
