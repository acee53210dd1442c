// kernel_border_forest.hip -- a round's border queue delivered to ALL subtrees of a forest inside ONE call (include/hpmvs_amd.h:
// hpmvs_border_forest_batch; reference CellProcessor.cpp:487-540).  Every rule is octree.hpp's; this file gives
// it lanes.  The tables are those launch_forest_build makes (kernel_extend_forest.hip): one buffer, a slot range per tree.
//
//   border_forest_static_kernel  one lane per patch: octree_route_kernel's loop over the roots, locate in the patch's OWN tree,
//                                the static refusal (written out at once, like an unrouted patch), the full path against that
//                                tree's root; sort keys = the static leaf's key and the tree id, 0 / 0 (no run) for a patch that
//                                is refused or unrouted
//   (rocPRIM radix_sort_pairs)   twice, both stable: by leaf key over 64 bits, then by tree id over ceil(log2 n_trees) bits (a
//                                leaf key fills 64 bits: the tree id cannot ride in it).  A run -- equal (tree, leaf key) -- ends up
//                                contiguous and in queue order
//   border_forest_gather_kernel  the keys of one array in the order of a sorted index array: the tree ids between the passes,
//                                and both keys behind the second, so that the replay reads its runs by position
//   border_forest_replay_kernel  octree_insert_replay_kernel's scheme, one wavefront per run: members 64 at a time, lcp_rank
//                                folded over the lane's own entries of A, a __shfl_xor butterfly, entry |A| appended by lane
//                                |A| mod 64.  The level widths are the run's own tree's: a table per WAVEFRONT in LDS (lane d
//                                writes level d), so the four wavefronts of a block serve four trees of different root widths
// No allocation and no launch size depends on data read back.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) border_forest_static_kernel(int n_trees, const octree::Tree* __restrict__ trees, int n,
                                                                   const float* __restrict__ center, const float* __restrict__ scale,
                                                                   BorderForestOut out, unsigned long long* __restrict__ path,
                                                                   unsigned long long* __restrict__ run_key,
                                                                   uint32_t* __restrict__ run_tree, uint32_t* __restrict__ sort_val) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {center[4 * (size_t)i], center[4 * (size_t)i + 1], center[4 * (size_t)i + 2]};
    const int32_t k = octree::route(n_trees, trees, p);
    sort_val[i] = (uint32_t)i;
    if (out.tree) out.tree[i] = k;
    bool refused = true;
    unsigned long long leaf = 0ull, pth = 0ull;
    if (k >= 0) {
        const octree::Tree tr = trees[k];
        const octree::Located l = octree::locate(tr.root, tr.t, p);
        refused = l.index != octree::kAbsent || l.cell.w < octree::border_add_width(scale[i]);   // add_target's own test
        leaf = l.key;
        if (!refused) pth = octree::full_path(tr.root, p);
    }
    run_key[i] = refused ? 0ull : leaf;
    run_tree[i] = refused ? 0u : (uint32_t)k;
    path[i] = pth;
    if (refused) {
        if (out.accepted) out.accepted[i] = 0;
        if (out.leaf_key) out.leaf_key[i] = leaf;
        if (out.blocker) out.blocker[i] = -1;
    }
}

// dst_x[pos] = src_x[order[pos]] for the arrays given (dst_key / src_key nullable)
__global__ void __launch_bounds__(256) border_forest_gather_kernel(int n, const uint32_t* __restrict__ order,
                                                                   const unsigned long long* __restrict__ src_key,
                                                                   const uint32_t* __restrict__ src_tree,
                                                                   unsigned long long* __restrict__ dst_key,
                                                                   uint32_t* __restrict__ dst_tree) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const uint32_t i = order[pos];
    if (dst_key) dst_key[pos] = src_key[i];
    dst_tree[pos] = src_tree[i];
}

__global__ void __launch_bounds__(256) border_forest_replay_kernel(const octree::Tree* __restrict__ trees, int n,
                                                                   const unsigned long long* __restrict__ run_key,
                                                                   const uint32_t* __restrict__ run_tree,
                                                                   const uint32_t* __restrict__ sort_val,
                                                                   const unsigned long long* __restrict__ path,
                                                                   const float* __restrict__ scale, unsigned long long* acc_key,
                                                                   int32_t* acc_owner, BorderForestOut out) {
#pragma clang fp contract(off)
    __shared__ float widths[4][64];   // a row per wavefront: [0 .. kMaxDepth] the level widths of the tree of the run it serves
    const int lane = threadIdx.x & 63;
    float* const width = widths[threadIdx.x >> 6];
    const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int pos = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); pos < n; pos += n_waves) {   // (wave-uniform)
        const unsigned long long run = run_key[pos];
        if (run == 0ull) continue;   // a refused or unrouted patch
        const uint32_t k = run_tree[pos];
        if (pos > 0 && run_key[pos - 1] == run && run_tree[pos - 1] == k) continue;   // not the head of its run: BOTH fields
        // level_widths(root width of tree k), level d by lane d: the chain Cell(parent, idx) makes
        float w = trees[k].root.w, mine = w;
        for (int d = 1; d <= octree::kMaxDepth; d++) {
            w = (float)((double)w / 2.0);
            if (lane == d) mine = w;
        }
        __builtin_amdgcn_wave_barrier();   // (the lanes are done with the table of the wave's previous run)
        if (lane <= octree::kMaxDepth) width[lane] = mine;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int leaf_depth = octree::key_depth(run);
        unsigned long long* const A = acc_key + pos;   // the run's slice: it holds at most as many entries as the run has members
        int32_t* const owner = acc_owner + pos;
        uint32_t count = 0;
        for (int m0 = pos;; m0 += 64) {
            const int m = m0 + lane;
            const bool mine_m = m < n && run_key[m] == run && run_tree[m] == k;   // (a run is contiguous: a prefix of the lanes)
            const int32_t my_i = mine_m ? (int32_t)sort_val[m] : 0;
            const unsigned long long my_path = mine_m ? path[my_i] : 0ull;
            const float my_a = mine_m ? octree::border_add_width(scale[my_i]) : 0.0f;
            const int members = __popcll(__ballot(mine_m));
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
                    if (out.accepted) out.accepted[i] = r.accepted ? 1 : 0;
                    if (out.leaf_key) out.leaf_key[i] = r.key;
                    if (out.blocker) out.blocker[i] = r.accepted ? -1 : best_owner;
                }
            }
            if (members < 64) break;
        }
    }
}

// bits of the tree-id pass: ids 0 .. n_trees - 1
static unsigned tree_bits(int n_trees) {
    unsigned b = 0;
    while (b < 31 && (1 << b) < n_trees) b++;
    return b;
}

size_t border_forest_temp_bytes(int n, int n_trees) {
    if (n <= 0) return 0;
    size_t a = 0, b = 0;
    if (rocprim::radix_sort_pairs(nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0u, 64u, (hipStream_t) nullptr) != hipSuccess)
        return (size_t)-1;
    const unsigned bits = tree_bits(n_trees);
    if (bits && rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                          (size_t)n, 0u, bits, (hipStream_t) nullptr) != hipSuccess)
        return (size_t)-1;
    if (b > a) a = b;
    return a ? a : 1;
}

int launch_border_forest(int n_trees, const octree::Tree* trees, int n, const float* center, const float* scale,
                         const BorderForestScratch& s, const BorderForestOut& out, hipStream_t st) {
    if (n <= 0) return 0;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(border_forest_static_kernel, grid, dim3(256), 0, st, n_trees, trees, n, center, scale, out, s.path, s.key_a, s.tree_a,
                       s.val_a);
    if (n_trees <= 0) return 0;   // (every patch is unrouted, and written out already)
    size_t bytes = s.temp_bytes;
    if (rocprim::radix_sort_pairs(s.temp, bytes, (const unsigned long long*)s.key_a, s.key_b, (const uint32_t*)s.val_a, s.val_b, (size_t)n, 0u,
                                  64u, st) != hipSuccess)
        return 1;
    const uint32_t* order = s.val_b;
    const unsigned bits = tree_bits(n_trees);
    if (bits) {   // (one tree: the first pass is the order already)
        hipLaunchKernelGGL(border_forest_gather_kernel, grid, dim3(256), 0, st, n, (const uint32_t*)s.val_b, (const unsigned long long*)nullptr,
                           (const uint32_t*)s.tree_a, (unsigned long long*)nullptr, s.tree_b);
        bytes = s.temp_bytes;
        if (rocprim::radix_sort_pairs(s.temp, bytes, (const uint32_t*)s.tree_b, s.tree_c, (const uint32_t*)s.val_b, s.val_a, (size_t)n, 0u, bits,
                                      st) != hipSuccess)
            return 1;
        order = s.val_a;
    }
    // both keys by sorted position (key_b and tree_b are free again)
    hipLaunchKernelGGL(border_forest_gather_kernel, grid, dim3(256), 0, st, n, order, (const unsigned long long*)s.key_a,
                       (const uint32_t*)s.tree_a, s.key_b, s.tree_b);
    // one wavefront per sorted position, up to 4096 blocks of four; the positions that head no run cost three loads
    const int blocks = (n + 3) / 4 < 4096 ? (n + 3) / 4 : 4096;
    hipLaunchKernelGGL(border_forest_replay_kernel, dim3((unsigned)blocks), dim3(256), 0, st, trees, n, (const unsigned long long*)s.key_b,
                       (const uint32_t*)s.tree_b, order, (const unsigned long long*)s.path, scale, s.acc_key, s.acc_owner, out);
    return 0;
}

}  // namespace hpmvs
