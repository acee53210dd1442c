// kernel_extend_tree.hip -- the two octree look-ups of CellProcessor::extend inside ONE expansion call (include/hpmvs_amd.h:
// hpmvs_extend_tree_batch).  Every rule is octree.hpp's (extend_pre / extend_post); this file only gives it lanes.
//
//   extend_tree_pre_kernel    one lane per candidate, right after expand_init_kernel: reads the centre that kernel wrote into the
//                             out batch (stride 4), decides the pre-gate (CellProcessor.cpp:122-125) and turns a skipped
//                             candidate's n_images into -20 -- what expand_init_kernel does with a skip byte it is handed -- so
//                             the refinement kernel passes it by (stage 20) and expand_gate_kernel restores 0
//   extend_tree_post_kernel   one lane per candidate, after expand_gate_kernel: the refined ones' (ok != 0) border test (:147)
//                             and addConditional's target leaf
// A lane reads 16 bytes of centre and writes at most 18; its cost is the chain of up to 21 dependent look-ups in a table that stays
// in L2, as in octree_locate_kernel.  Both kernels write every entry of every output they are given.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) extend_tree_pre_kernel(octree::Cell root, octree::Table t, int n, float width, float add_width,
                                                              const float* __restrict__ center, int32_t* __restrict__ n_images,
                                                              ExtendTreeOut out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
    const octree::ExtendPre r = octree::extend_pre(root, t, p, width, add_width);
    if (out.skip) out.skip[i] = r.skip ? 1 : 0;
    if (out.pre_inside) out.pre_inside[i] = r.inside ? 1 : 0;
    if (out.pre_key) out.pre_key[i] = r.pre_key;
    if (r.skip && n_images[i] > 0) n_images[i] = -20;
}

__global__ void __launch_bounds__(256) extend_tree_post_kernel(octree::Cell root, octree::Table t, int n, float add_width,
                                                               const float* __restrict__ center, const uint8_t* __restrict__ ok,
                                                               ExtendTreeOut out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    octree::ExtendPost r{false, 0};
    if (ok[i]) {
        const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
        r = octree::extend_post(root, t, p, add_width);
    }
    if (out.border) out.border[i] = r.border ? 1 : 0;
    if (out.post_key) out.post_key[i] = r.post_key;
}

void launch_extend_tree_pre(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n, float width,
                            const DevBatch& out, const ExtendTreeOut& k, hipStream_t st) {
    if (n <= 0) return;
    const octree::Cell r{{root[0], root[1], root[2]}, root[3]};
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    hipLaunchKernelGGL(extend_tree_pre_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r, t, n, width,
                       octree::extend_add_width(width), out.center, out.n_images, k);
}

void launch_extend_tree_post(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n, float width,
                             const DevBatch& out, const ExtendTreeOut& k, hipStream_t st) {
    if (n <= 0) return;
    const octree::Cell r{{root[0], root[1], root[2]}, root[3]};
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    hipLaunchKernelGGL(extend_tree_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r, t, n,
                       octree::extend_add_width(width), out.center, out.ok, k);
}

}  // namespace hpmvs
