// kernel_regularize.hip -- CellProcessor::regularize (reference src/hpmvs/CellProcessor.cpp:309-367) for a whole priority level
// against a VERSIONED snapshot of the scheduler's octree.
//
// The snapshot is a table of the nonempty leaves: per leaf its Cell::c_ / width_, the centre of data[0] and the queue positions
// born < q < died between which it exists.  regularize_leaf_kernel re-derives every leaf's path from the root with the reference's
// recurrences (Cell(parent, idx), doctree.cpp:30-36: double arithmetic, float storage; Branch::at, doctree.h:250-255: child
// x > c_), checks that the recomputed centre is the one passed in and enters the path key (3 bits per level below a sentinel bit)
// into an open-addressing hash table.  regularize_kernel then follows regularize for every cell: 24 probes descend from the root
// through the same recurrences and take the first leaf on their path that is valid at the cell's queue position.
//
// Shape: one lane per (cell, probe), 32 lanes per cell (24 probing), 8 cells per 256-lane workgroup.  A probe is a chain of up
// to 21 dependent hash look-ups (global loads, L2 or HBM latency); one lane per cell would serialise 24 such chains per lane and
// leave ~1.5 waves per SIMD at 1e5 cells, far below the 8 that hide memory latency.  The distinct leaves are found across lanes
// through LDS; the squared plane distances are computed by the lanes that own a first occurrence and summed by the cell's first
// lane in first-probe order (yy outer, xx inner), which is where this path may differ from a given reference run: the reference
// sums over a std::set<Leaf*>, in heap-address order.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "photometric.hpp"

namespace hpmvs {

__device__ __forceinline__ unsigned long long reg_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// Cell(parent, idx): width_ = parent width / 2.0, c_[k] = parent c_[k] + (+-1.0) * width_ / 2.0, in double, stored as float
__device__ __forceinline__ void reg_child(float* c, float& w, const float* p) {
    const float cw = (float)((double)w / 2.0);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = (float)((double)c[k] + ((p[k] > c[k]) ? 1.0 : -1.0) * (double)cw / 2.0);
    w = cw;
}
__device__ __forceinline__ unsigned reg_octant(const float* c, const float* p) {
    return ((unsigned)(p[2] > c[2]) << 2) | ((unsigned)(p[1] > c[1]) << 1) | (unsigned)(p[0] > c[0]);
}

// per leaf: path key, checks, hash insertion.  hdr[0] |= 1: a leaf off the grid or deeper than kRegMaxDepth; hdr[0] |= 2: an
// expanded cell whose reference image is not a view of the scene; hdr[1] = deepest leaf; hdr[2] = kRegMaxDepth + 1 - shallowest leaf.
__global__ void __launch_bounds__(256) regularize_leaf_kernel(RegTree t, int n_cells, int n_views, const int32_t* __restrict__ ref,
                                                              int ref_stride, const int32_t* __restrict__ n_images,
                                                              const uint8_t* __restrict__ expanded, int32_t* hdr) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cells && expanded[i]) {
        const int r = ref[(size_t)i * ref_stride];
        if ((n_images && n_images[i] < 1) || r < 0 || r >= n_views) atomicOr(&hdr[0], 2);
    }
    if (i >= t.n) return;
    const float lc[3] = {t.cell_center[3 * i], t.cell_center[3 * i + 1], t.cell_center[3 * i + 2]};
    const float lw = t.cell_width[i];
    float c[3] = {t.root[0], t.root[1], t.root[2]};
    float w = t.root[3];
    unsigned long long key = 1;
    int d = 0;
    bool bad = false;
    while (!(w == lw)) {
        if (d == kRegMaxDepth) { bad = true; break; }
        key = (key << 3) | reg_octant(c, lc);
        reg_child(c, w, lc);
        d++;
    }
    if (!bad)
        bad = d == 0 || __float_as_uint(c[0]) != __float_as_uint(lc[0]) || __float_as_uint(c[1]) != __float_as_uint(lc[1]) ||
              __float_as_uint(c[2]) != __float_as_uint(lc[2]);
    if (bad) { atomicOr(&hdr[0], 1); return; }
    atomicMax(&hdr[1], d);
    atomicMax(&hdr[2], kRegMaxDepth + 1 - d);
    const unsigned long long mask = (unsigned long long)t.slots - 1;
    unsigned long long h = reg_hash(key) & mask;
    while (true) {   // slots >= 2 n: a free slot exists
        const unsigned long long prev = atomicCAS(&t.keys[h], 0ull, key);
        if (prev == 0ull) { t.vals[h] = i; break; }
        h = (h + 1) & mask;
    }
}

// the first leaf of `key`'s slot chain that exists at queue position q, else -1
__device__ __forceinline__ int reg_lookup(const RegTree& t, unsigned long long key, int q) {
    const unsigned long long mask = (unsigned long long)t.slots - 1;
    unsigned long long h = reg_hash(key) & mask;
    while (true) {
        const unsigned long long k = t.keys[h];
        if (k == 0ull) return -1;
        if (k == key) {
            const int v = t.vals[h];
            if (t.born[v] < q && q < t.died[v]) return v;
        }
        h = (h + 1) & mask;
    }
}

constexpr int kRegLanes = 32;    // lanes per cell (probes 0..23 active)
constexpr int kRegCells = 8;     // cells per workgroup

__global__ void __launch_bounds__(256) regularize_kernel(DevScene sc, RegTree t, RegCells cl, int min_depth, int max_depth) {
#pragma clang fp contract(off)
    __shared__ int s_leaf[256];
    __shared__ float s_err[256];
    const int lane = threadIdx.x & (kRegLanes - 1);
    const int g = threadIdx.x / kRegLanes;
    const int i = blockIdx.x * kRegCells + g;
    const bool live = i < cl.n && cl.expanded[i];
    int leaf = -1;
    float nn[3] = {0.f, 0.f, 0.f}, x0[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float pn[3] = {cl.normal[4 * i], cl.normal[4 * i + 1], cl.normal[4 * i + 2]};
        x0[0] = cl.center[4 * i]; x0[1] = cl.center[4 * i + 1]; x0[2] = cl.center[4 * i + 2];
        normalized3f(pn, nn);
        if (lane < 24) {
            const DevView& V = sc.views[cl.ref[(size_t)i * cl.ref_stride]];
            float t0[3], yaxis[3], xaxis[3];
            cross3f(pn, V.xaxis, t0);
            normalized3f(t0, yaxis);
            cross3f(yaxis, pn, xaxis);
            const int k = lane < 12 ? lane : lane + 1;   // (0, 0) skipped; yy outer, xx inner
            const float fy = (float)(k / 5 - 2), fx = (float)(k % 5 - 2);
            const float width = cl.width[i];
            float p[3];
#pragma unroll
            for (int j = 0; j < 3; j++) p[j] = x0[j] + (fx * xaxis[j] + fy * yaxis[j]) * width;
            const int q = cl.position[i];
            float c[3] = {t.root[0], t.root[1], t.root[2]};
            float w = t.root[3];
            unsigned long long key = 1;
            for (int d = 1; d <= max_depth && leaf < 0; d++) {   // no leaf lies above min_depth: no look-up there
                key = (key << 3) | reg_octant(c, p);
                reg_child(c, w, p);
                if (d >= min_depth) leaf = reg_lookup(t, key, q);
            }
        }
    }
    s_leaf[threadIdx.x] = leaf;
    __syncthreads();
    const int base = g * kRegLanes;
    bool first = leaf >= 0;
    for (int j = 0; j < lane && first; j++) first = s_leaf[base + j] != leaf;
    float err2 = 0.f;
    if (first) {
        const float b[3] = {t.patch_center[3 * leaf] - x0[0], t.patch_center[3 * leaf + 1] - x0[1], t.patch_center[3 * leaf + 2] - x0[2]};
        const float e = dot3f(nn, b);
        err2 = e * e;
    }
    s_err[threadIdx.x] = first ? err2 : -1.f;   // -1: not a first occurrence
    __syncthreads();
    if (lane != 0 || i >= cl.n) return;
    int32_t* row = cl.neighbour ? cl.neighbour + (size_t)i * 24 : nullptr;
    if (!cl.expanded[i]) {   // regularize returns before anything (flatness_ unchanged)
        cl.n_neighbours[i] = -1;
        if (row) for (int j = 0; j < 24; j++) row[j] = -1;
        return;
    }
    int cnt = 0;
    float dist = 0.f;
    for (int j = 0; j < 24; j++) {
        const float e2 = s_err[base + j];
        if (e2 < 0.f) continue;
        if (row) row[cnt] = s_leaf[base + j];
        dist += e2;
        cnt++;
    }
    if (row) for (int j = cnt; j < 24; j++) row[j] = -1;
    cl.n_neighbours[i] = cnt;
    float f;
    if (cnt < 1) f = 2.6f;
    else if (cnt < 4) f = 2.5f;
    else f = sqrtf(dist / (float)cnt) / cl.width[i];
    cl.flatness[i] = f;
}

void launch_regularize_leaves(const RegTree& t, int n_cells, int n_views, const int32_t* ref, int ref_stride, const int32_t* n_images,
                              const uint8_t* expanded, int32_t* hdr, hipStream_t st) {
    const int n = t.n > n_cells ? t.n : n_cells;
    if (n <= 0) return;
    hipLaunchKernelGGL(regularize_leaf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, n_cells, n_views, ref, ref_stride,
                       n_images, expanded, hdr);
}

void launch_regularize(const DevScene& sc, const RegTree& t, const RegCells& cl, int min_depth, int max_depth, hipStream_t st) {
    if (cl.n <= 0) return;
    hipLaunchKernelGGL(regularize_kernel, dim3((unsigned)((cl.n + kRegCells - 1) / kRegCells)), dim3(256), 0, st, sc, t, cl, min_depth,
                       max_depth);
}

}  // namespace hpmvs
