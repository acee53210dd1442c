// kernel_octree_insert.hip -- a round's border patches routed to their subtrees and inserted in queue order, as ONE call each
// (include/hpmvs_amd.h: hpmvs_octree_route_batch, hpmvs_octree_insert_batch; reference CellProcessor.cpp:487-540; DESIGN.md
// §3.12).  Every rule is octree.hpp's; this file gives it lanes.
//
//   octree_route_kernel          one lane per point over the subtree roots (uniform loads of [n_trees][4] floats): the first root
//                                in list order whose contains(p) holds, -1 when none does
//   octree_insert_static_kernel  one lane per patch: locate in the unchanged tree, the static refusal (written out at once),
//                                the full path; sort key = the static leaf's key, 0 (no key) for a refused patch
//   (rocPRIM radix_sort_pairs)   stable: the queue order survives inside a run of equal static leaf
//   octree_insert_replay_kernel  one wavefront per run.  The members are taken 64 at a time (one per lane, handed round by
//                                shuffle), each in queue order against the run's accepted list A: lane l holds the entries
//                                j = l (mod 64) of A, folds lcp_rank over them, a 6-step butterfly gives EVERY lane the maximum
//                                and its owner, every lane takes insert_decide (wave-uniform), and entry |A| is appended by lane
//                                |A| mod 64 -- so a lane only ever reads entries of A that it stored itself, and the list needs
//                                no hand-over between lanes through memory.  A is a slice of a scratch array as long as the run
//                                (at its sorted position): no allocation depends on data.  g members cost O(g |A| / 64) steps.
#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) octree_route_kernel(int n_trees, const float* __restrict__ roots, int n,
                                                           const float* __restrict__ points, int32_t* __restrict__ tree) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    int32_t found = -1;
    for (int t = 0; t < n_trees; t++) {
        const octree::Cell r{{roots[4 * (size_t)t], roots[4 * (size_t)t + 1], roots[4 * (size_t)t + 2]}, roots[4 * (size_t)t + 3]};
        if (octree::contains(r, p)) { found = t; break; }
    }
    tree[i] = found;
}

__global__ void __launch_bounds__(256) octree_insert_static_kernel(octree::Cell root, octree::Table t, int n, const float* __restrict__ points,
                                                                   const float* __restrict__ add_width, OctreeInsertOut out,
                                                                   unsigned long long* __restrict__ path,
                                                                   unsigned long long* __restrict__ sort_key,
                                                                   uint32_t* __restrict__ sort_val) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    const float a = add_width[i];
    const octree::Located l = octree::locate(root, t, p);
    const bool refused = l.index != octree::kAbsent || l.cell.w < a;   // add_target's own test
    sort_val[i] = (uint32_t)i;
    sort_key[i] = refused ? 0ull : l.key;
    path[i] = refused ? 0ull : octree::full_path(root, p);
    if (refused) {
        out.accepted[i] = 0;
        out.leaf_key[i] = l.key;
        if (out.blocker) out.blocker[i] = -1;
    }
}

__global__ void __launch_bounds__(256) octree_insert_replay_kernel(float root_width, int n, const unsigned long long* __restrict__ sort_key,
                                                                   const uint32_t* __restrict__ sort_val,
                                                                   const unsigned long long* __restrict__ path,
                                                                   const float* __restrict__ add_width, unsigned long long* acc_key,
                                                                   int32_t* acc_owner, OctreeInsertOut out) {
#pragma clang fp contract(off)
    __shared__ float width[octree::kMaxDepth + 1];
    if (threadIdx.x == 0) {
        const octree::Widths W = octree::level_widths(root_width);
        for (int d = 0; d <= octree::kMaxDepth; d++) width[d] = W.w[d];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int pos = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); pos < n; pos += n_waves) {   // (wave-uniform)
        const unsigned long long run = sort_key[pos];
        if (run == 0ull || (pos > 0 && sort_key[pos - 1] == run)) continue;   // a refused patch, or not the head of its run
        const int leaf_depth = octree::key_depth(run);
        unsigned long long* const A = acc_key + pos;   // the run's slice: it holds at most as many entries as the run has members
        int32_t* const owner = acc_owner + pos;
        uint32_t count = 0;
        for (int m0 = pos;; m0 += 64) {
            const int m = m0 + lane;
            const bool mine = m < n && sort_key[m] == run;   // (a run is contiguous: the lanes that hold a member are a prefix)
            const int32_t my_i = mine ? (int32_t)sort_val[m] : 0;
            const unsigned long long my_path = mine ? path[my_i] : 0ull;
            const float my_a = mine ? add_width[my_i] : 0.0f;
            const int members = __popcll(__ballot(mine));
            for (int s = 0; s < members; s++) {
                const int32_t i = __shfl(my_i, s);
                const unsigned long long pth = __shfl(my_path, s);
                const float a = __shfl(my_a, s);
                unsigned long long best = 0ull;
                int32_t best_owner = -1;
                for (uint32_t j = (uint32_t)lane; j < count; j += 64) {
                    const unsigned long long r = octree::lcp_rank(pth, A[j], j);
                    if (r > best) { best = r; best_owner = owner[j]; }
                }
                for (int off = 32; off >= 1; off >>= 1) {   // ranks are distinct (the position is in them): every lane ends equal
                    const unsigned long long o = __shfl_xor(best, off);
                    const int32_t oo = __shfl_xor(best_owner, off);
                    if (o > best) { best = o; best_owner = oo; }
                }
                const octree::Inserted r = octree::insert_decide(leaf_depth, pth, a, width, count > 0, octree::rank_lcp(best), octree::rank_hit(best));
                if (r.accepted) {
                    if (lane == (int)(count & 63u)) { A[count] = r.key; owner[count] = i; }
                    count++;
                }
                if (lane == 0) {
                    out.accepted[i] = r.accepted ? 1 : 0;
                    out.leaf_key[i] = r.key;
                    if (out.blocker) out.blocker[i] = r.accepted ? -1 : best_owner;
                }
            }
            if (members < 64) break;
        }
    }
}

void launch_octree_route(int n_trees, const float* roots, int n, const float* points, int32_t* tree, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(octree_route_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n_trees, roots, n, points, tree);
}

size_t octree_insert_temp_bytes(int n) {
    size_t bytes = 0;
    if (n <= 0) return 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0u, 64u, (hipStream_t) nullptr) != hipSuccess)
        return (size_t)-1;
    return bytes ? bytes : 1;
}

int launch_octree_insert(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n,
                         const float* points, const float* add_width, const OctreeInsertScratch& s, const OctreeInsertOut& out,
                         hipStream_t st) {
    if (n <= 0) return 0;
    const octree::Cell r{{root[0], root[1], root[2]}, root[3]};
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    hipLaunchKernelGGL(octree_insert_static_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r, t, n, points, add_width, out,
                       s.path, s.key_a, s.val_a);
    size_t bytes = s.temp_bytes;
    if (rocprim::radix_sort_pairs(s.temp, bytes, (const unsigned long long*)s.key_a, s.key_b, (const uint32_t*)s.val_a, s.val_b, (size_t)n, 0u,
                                  64u, st) != hipSuccess)
        return 1;
    // one wavefront per sorted position, up to 4096 blocks of four; the positions that head no run cost two loads
    const int blocks = (n + 3) / 4 < 4096 ? (n + 3) / 4 : 4096;
    hipLaunchKernelGGL(octree_insert_replay_kernel, dim3((unsigned)blocks), dim3(256), 0, st, root[3], n, (const unsigned long long*)s.key_b,
                       (const uint32_t*)s.val_b, (const unsigned long long*)s.path, add_width, s.acc_key, s.acc_owner, out);
    return 0;
}

}  // namespace hpmvs
