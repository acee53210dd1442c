// kernel_filter.hip -- CellProcessor::filter (reference src/hpmvs/CellProcessor.cpp:43-82) for every cell of a priority level
// (DESIGN.md §3.9).  filter reads only the cell's own patches (no map, no tree, no image), so every cell's decision is known up
// front; the losers' subtractions are one ordered hpmvs_depth_ops_batch afterwards.
//
// filter_dist_kernel: one lane per patch row.  The lane finds its cell by binary search in cell_start and runs the reference's
// inner loop for its row: n = normalized(normal), x0 = centre, dist += n . (c_jj - x0) for jj != ii in data order, then
// dist / (float)(k - 1).  Every per-row sum is sequential in jj, so `dist` is the reference's float bit for bit.  The lanes of
// one cell read the same centre at the same step (one L1 line serves the wave); a cell of k patches costs k steps on each of its
// k lanes, so the launch takes as long as its largest cell, not as the sum of the cells.
//
// filter_keep_kernel: one wavefront per cell.  The reference keeps the first ii with dist < best, best starting at FLT_MAX: the
// lowest index reaching the minimum among the values < FLT_MAX (NaN and +inf never compare below).  Each lane scans its
// strided share in increasing order with the same strict test, then the wave reduces (value, index) pairs by value, ties to
// the lower index; on values that are not NaN that is a total order, so the minimum -- and the kept row -- do not depend on the
// reduction's shape.  A cell of thousands of rows is 64 loads deep per lane instead of thousands.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "launch.h"
#include "photometric.hpp"

namespace hpmvs {

// cell_start[0] == 0, non-decreasing, cell_start[n_cells] == n; bad[0] |= 1 otherwise
__global__ void __launch_bounds__(256) filter_check_kernel(const int32_t* __restrict__ cell_start, int n_cells, int n, int32_t* bad) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_cells) return;
    const int v = cell_start[c];
    bool ok = true;
    if (c == 0) ok = v == 0;
    else ok = v >= cell_start[c - 1];
    if (c == n_cells) ok = ok && v == n;
    if (!ok) atomicOr(bad, 1);
}

__global__ void __launch_bounds__(256) filter_dist_kernel(const float* __restrict__ center, const float* __restrict__ normal,
                                                          const int32_t* __restrict__ cell_start, int n_cells, int n,
                                                          float* __restrict__ dist) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    // the cell of row r: the last c with cell_start[c] <= r (empty cells have equal offsets; cell_start[n_cells] = n > r)
    int lo = 0, hi = n_cells;   // cell_start[lo] <= r < cell_start[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (cell_start[mid] <= r) lo = mid;
        else hi = mid;
    }
    const int s = cell_start[lo], e = cell_start[lo + 1];
    const int k = e - s;
    if (k < 2) { dist[r] = 0.0f; return; }   // filter returns before anything for a single patch
    const float pn[3] = {normal[4 * (size_t)r], normal[4 * (size_t)r + 1], normal[4 * (size_t)r + 2]};
    const float x0[3] = {center[4 * (size_t)r], center[4 * (size_t)r + 1], center[4 * (size_t)r + 2]};
    float nn[3];
    normalized3f(pn, nn);
    float d = 0.0f;
    for (int j = s; j < e; j++) {
        if (j == r) continue;
        const float b[3] = {center[4 * (size_t)j] - x0[0], center[4 * (size_t)j + 1] - x0[1], center[4 * (size_t)j + 2] - x0[2]};
        d += dot3f(nn, b);
    }
    dist[r] = d / (float)(k - 1);
}

constexpr int kFilterWave = 64;

__global__ void __launch_bounds__(256) filter_keep_kernel(const float* __restrict__ dist, const int32_t* __restrict__ cell_start,
                                                          int n_cells, int32_t* __restrict__ keep) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kFilterWave - 1);
    const int c = blockIdx.x * (blockDim.x / kFilterWave) + threadIdx.x / kFilterWave;
    if (c >= n_cells) return;   // (uniform per wave)
    const int s = cell_start[c], e = cell_start[c + 1];
    const int k = e - s;
    if (k < 2) {
        if (lane == 0) keep[c] = k == 1 ? s : -1;
        return;
    }
    float best = FLT_MAX;
    int idx = INT_MAX;   // none yet
    for (int j = s + lane; j < e; j += kFilterWave) {
        const float d = dist[j];
        if (d < best) { best = d; idx = j; }
    }
#pragma unroll
    for (int m = kFilterWave / 2; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, kFilterWave);
        const int oi = __shfl_xor(idx, m, kFilterWave);
        if (oi != INT_MAX && (idx == INT_MAX || ob < best || (ob == best && oi < idx))) { best = ob; idx = oi; }
    }
    if (lane == 0) keep[c] = idx == INT_MAX ? -2 : idx;
}

void launch_filter_check(const int32_t* cell_start, int n_cells, int n, int32_t* bad, hipStream_t st) {
    hipLaunchKernelGGL(filter_check_kernel, dim3((unsigned)((n_cells + 1 + 255) / 256)), dim3(256), 0, st, cell_start, n_cells, n, bad);
}

void launch_filter(const float* center, const float* normal, const int32_t* cell_start, int n_cells, int n, float* dist, int32_t* keep,
                   hipStream_t st) {
    if (n > 0)
        hipLaunchKernelGGL(filter_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, center, normal, cell_start, n_cells, n,
                           dist);
    if (n_cells > 0) {
        const int per = 256 / kFilterWave;
        hipLaunchKernelGGL(filter_keep_kernel, dim3((unsigned)((n_cells + per - 1) / per)), dim3(256), 0, st, dist, cell_start, n_cells,
                           keep);
    }
}

}  // namespace hpmvs
