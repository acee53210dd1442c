// kernel_process_forest.hip -- one regularize / settle sweep of processCell over ALL subtrees of a partition (include/hpmvs_amd.h:
// hpmvs_process_forest_batch).  Every rule is octree.hpp's; this file only gives it lanes.  The tables are those
// of forest_build_kernel / forest_check_kernel (kernel_extend_forest.hip).
//
//   process_cell_kernel        one lane per cell: its tree, its leaf by a look-up of its key, the claim of that leaf (the lowest
//                              row wins), the cell's c_ / width_ by Cell(parent, idx) down the key, the row's checks
//   process_claim_kernel       one lane per cell, behind all claims: a row that does not own its leaf names a leaf claimed twice
//   process_skip_kernel        one lane per cell, behind level_support: removed, and the skip bytes of its four children
//   process_decide_kernel      one lane per cell, behind expand_gate: children, split, child keys, setDepths calls of the cell
//   process_gather_kernel      one lane per cell, behind the exclusive scan of the counts: the op rows and their subtract bytes
//   regularize_forest_kernel   regularize_kernel's lane shape: 32 lanes per cell (24 probing), 8 cells per 256-lane workgroup, the
//                              distinct leaves found through LDS by their keys, the sum by the cell's first lane
// The claim is an atomicMin and not a compare-and-swap: whichever of three rows on one leaf came first, the row that is refused
// is the second LOWEST, which is what "the lowest offender" means on every run.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) process_cell_kernel(int n_trees, const octree::Tree* __restrict__ trees,
                                                           const int32_t* __restrict__ leaf_first, int n_views, ProcessCells c,
                                                           uint32_t* verdict) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    c.gleaf[i] = -1;
    const int32_t k = c.cell_tree[i];
    if (k < 0 || k >= n_trees) { atomicMin(&verdict[kForestParent], octree::cell_finding(i, octree::kCellTree)); return; }
    const uint64_t key = c.cell_key[i];
    const int depth = octree::key_depth(key);
    const int32_t idx = depth < 1 || depth > octree::kMaxDepth ? octree::kAbsent : octree::find(trees[k].t, key);
    if (idx < 0) { atomicMin(&verdict[kForestParent], octree::cell_finding(i, octree::kCellLeaf)); return; }
    const int32_t g = leaf_first[k] + idx;
    c.gleaf[i] = g;
    atomicMin(&c.owner[g], i);
    const float f = c.flatness[i];
    const bool reg = octree::process_regularized(f);
    if (!reg && !octree::process_removed(f) && depth >= octree::kMaxDepth)
        atomicMin(&verdict[kForestParent], octree::cell_finding(i, octree::kCellDeep));
    if (reg) {
        const int r = c.images[(size_t)i * c.max_images];
        if (c.n_images[i] < 1 || r < 0 || r >= n_views) atomicMin(&verdict[kForestParent], octree::cell_finding(i, octree::kCellRef));
    }
    const octree::Cell cell = octree::key_cell(trees[k].root, key);
    c.cell_center[3 * (size_t)i] = cell.c[0]; c.cell_center[3 * (size_t)i + 1] = cell.c[1]; c.cell_center[3 * (size_t)i + 2] = cell.c[2];
    c.cell_width[i] = cell.w;
}

__global__ void __launch_bounds__(256) process_claim_kernel(ProcessCells c, uint32_t* verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const int32_t g = c.gleaf[i];
    if (g >= 0 && c.owner[g] != i) atomicMin(&verdict[kForestParent], octree::cell_finding(i, octree::kCellTwice));
}

__global__ void __launch_bounds__(256) process_skip_kernel(ProcessCells c, const int32_t* __restrict__ support, uint8_t* __restrict__ skip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const float f = c.flatness[i];
    const bool reg = octree::process_regularized(f), removed = !reg && octree::process_removed(f);
    c.removed[i] = removed ? 1 : 0;
    const uint8_t s = (reg || removed || support[i] < 1) ? 1 : 0;
    for (int k = 0; k < 4; k++) skip[4 * (size_t)i + k] = s;
}

__global__ void __launch_bounds__(256) process_decide_kernel(ProcessCells c, const int32_t* __restrict__ support,
                                                             const uint8_t* __restrict__ skip, const uint8_t* __restrict__ final_level,
                                                             const uint8_t* __restrict__ child_ok, const float* __restrict__ child_center,
                                                             int32_t* __restrict__ op_count) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const bool reg = octree::process_regularized(c.flatness[i]), removed = c.removed[i] != 0;
    const octree::Cell cell{{c.cell_center[3 * (size_t)i], c.cell_center[3 * (size_t)i + 1], c.cell_center[3 * (size_t)i + 2]}, c.cell_width[i]};
    int nc = 0;
    for (int k = 0; k < 4; k++) {
        const size_t t = 4 * (size_t)i + k;
        const bool ch = !skip[t] && child_ok[t] != 0;
        c.children[t] = ch ? 1 : 0;
        const float p[3] = {child_center[4 * t], child_center[4 * t + 1], child_center[4 * t + 2]};
        c.child_key[t] = ch ? octree::process_child_key(c.cell_key[i], cell, p) : 0ull;
        nc += ch ? 1 : 0;
    }
    const bool split = !reg && octree::process_split(removed, support[i], final_level[i] != 0, nc);
    c.split[i] = split ? 1 : 0;
    op_count[i] = reg ? 0 : octree::process_op_count(removed, split, nc);
}

// op_first: the exclusive scan of op_count.  The op rows are wide copies of the patches: centre, normal, scale, list.
__global__ void __launch_bounds__(256) process_gather_kernel(ProcessCells c, const int32_t* __restrict__ op_first, DevBatch par, DevBatch out,
                                                             DevBatch ops, uint8_t* __restrict__ subtract) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    if (!c.removed[i] && !c.split[i]) return;
    int o = op_first[i];
    for (int k = -1; k < 4; k++) {
        if (k >= 0 && !(c.split[i] && c.children[4 * (size_t)i + k])) continue;
        const DevBatch& src = k < 0 ? par : out;
        const size_t t = k < 0 ? (size_t)i : 4 * (size_t)i + k;
        for (int j = 0; j < 4; j++) { ops.center[4 * (size_t)o + j] = src.center[4 * t + j]; ops.normal[4 * (size_t)o + j] = src.normal[4 * t + j]; }
        ops.scale[o] = src.scale[t];
        const int nimg = src.n_images[t];
        ops.n_images[o] = nimg;
        for (int j = 0; j < ops.max_images; j++)
            ops.images[(size_t)o * ops.max_images + j] = (j < nimg && j < src.max_images) ? src.images[t * src.max_images + j] : -1;
        subtract[o] = k < 0 ? 1 : 0;
        o++;
    }
}

constexpr int kRegLanes = 32;    // lanes per cell (probes 0..23 active)
constexpr int kRegCells = 8;     // cells per workgroup

__global__ void __launch_bounds__(256) regularize_forest_kernel(DevScene sc, const octree::Tree* __restrict__ trees,
                                                                const int32_t* __restrict__ leaf_first,
                                                                const float* __restrict__ leaf_patch_center, ProcessCells c, DevBatch par,
                                                                const float* __restrict__ child_center, float* flatness_out,
                                                                int32_t* __restrict__ n_neighbours,
                                                                unsigned long long* __restrict__ neighbour_key) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_key[256];
    __shared__ float s_err[256];
    const int lane = threadIdx.x & (kRegLanes - 1);
    const int g = threadIdx.x / kRegLanes;
    const int i = blockIdx.x * kRegCells + g;
    const bool live = i < c.n && octree::process_regularized(c.flatness[i]);
    unsigned long long key = 0ull;   // 0: the probe found no nonempty leaf
    const float* pc = nullptr;
    float nn[3] = {0.f, 0.f, 0.f}, x0[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float pn[3] = {par.normal[4 * (size_t)i], par.normal[4 * (size_t)i + 1], par.normal[4 * (size_t)i + 2]};
        x0[0] = par.center[4 * (size_t)i]; x0[1] = par.center[4 * (size_t)i + 1]; x0[2] = par.center[4 * (size_t)i + 2];
        octree::ot_normalized3(pn, nn);
        if (lane < 24) {
            const DevView& V = sc.views[par.images[(size_t)i * par.max_images]];
            float p[3];
            octree::regularize_probe(x0, pn, V.xaxis, c.cell_width[i], lane, p);
            const int32_t k = c.cell_tree[i];
            const octree::Sweep sw{c.owner, c.removed, c.split, c.children, (const uint64_t*)c.child_key};
            const octree::Probe pr = octree::locate_versioned(trees[k], leaf_first[k], sw, i, p);
            if (pr.child >= 0) { key = pr.key; pc = child_center + 4 * (size_t)pr.child; }
            else if (pr.leaf != octree::kAbsent) { key = pr.key; pc = leaf_patch_center + 3 * (size_t)pr.leaf; }
        }
    }
    s_key[threadIdx.x] = key;
    __syncthreads();
    const int base = g * kRegLanes;
    bool first = key != 0ull;
    for (int j = 0; j < lane && first; j++) first = s_key[base + j] != key;
    s_err[threadIdx.x] = first ? octree::regularize_err2(nn, x0, pc) : -1.f;   // -1: not a first occurrence
    __syncthreads();
    if (lane != 0 || i >= c.n) return;
    unsigned long long* row = neighbour_key ? neighbour_key + (size_t)i * 24 : nullptr;
    if (!live) {   // a settled cell
        if (n_neighbours) n_neighbours[i] = -2;
        if (row) for (int j = 0; j < 24; j++) row[j] = 0ull;
        return;
    }
    int cnt = 0;
    float dist = 0.f;
    for (int j = 0; j < 24; j++) {
        const float e2 = s_err[base + j];
        if (e2 < 0.f) continue;
        if (row) row[cnt] = s_key[base + j];
        dist += e2;
        cnt++;
    }
    if (row) for (int j = cnt; j < 24; j++) row[j] = 0ull;
    if (n_neighbours) n_neighbours[i] = cnt;
    flatness_out[i] = octree::regularize_flatness(cnt, dist, c.cell_width[i]);
}

static dim3 grid_of(int n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_process_cells(int n_trees, const octree::Tree* trees, const int32_t* leaf_first, int n_views, const ProcessCells& c,
                          uint32_t* verdict, hipStream_t st) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(process_cell_kernel, grid_of(c.n), dim3(256), 0, st, n_trees, trees, leaf_first, n_views, c, verdict);
    hipLaunchKernelGGL(process_claim_kernel, grid_of(c.n), dim3(256), 0, st, c, verdict);
}
void launch_process_skip(const ProcessCells& c, const int32_t* support, uint8_t* skip, hipStream_t st) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(process_skip_kernel, grid_of(c.n), dim3(256), 0, st, c, support, skip);
}
void launch_process_decide(const ProcessCells& c, const int32_t* support, const uint8_t* skip, const uint8_t* final_level, const DevBatch& out,
                           int32_t* op_count, hipStream_t st) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(process_decide_kernel, grid_of(c.n), dim3(256), 0, st, c, support, skip, final_level, out.ok, out.center, op_count);
}
int process_scan(void* temp, size_t* temp_bytes, const int32_t* in, int32_t* out, int n, hipStream_t st) {
    return (int)rocprim::exclusive_scan(temp, *temp_bytes, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st);
}
void launch_process_gather(const ProcessCells& c, const int32_t* op_first, const DevBatch& par, const DevBatch& out, const DevBatch& ops,
                           uint8_t* subtract, hipStream_t st) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(process_gather_kernel, grid_of(c.n), dim3(256), 0, st, c, op_first, par, out, ops, subtract);
}
void launch_regularize_forest(const DevScene& sc, const octree::Tree* trees, const int32_t* leaf_first, const float* leaf_patch_center,
                              const ProcessCells& c, const DevBatch& par, const DevBatch& out, float* flatness_out, int32_t* n_neighbours,
                              unsigned long long* neighbour_key, hipStream_t st) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(regularize_forest_kernel, dim3((unsigned)((c.n + kRegCells - 1) / kRegCells)), dim3(256), 0, st, sc, trees, leaf_first,
                       leaf_patch_center, c, par, out.center, flatness_out, n_neighbours, neighbour_key);
}

}  // namespace hpmvs
