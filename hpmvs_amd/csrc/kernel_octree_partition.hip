// kernel_octree_partition.hip -- the octree split into subtrees as main's getSubTrees does it, and cellHistogram, as ONE call
// (include/hpmvs_amd.h: hpmvs_octree_partition; reference src/main.cpp:50-96, doctree.h:236-247, 493-523).
// Every rule is octree.hpp's; this file gives it lanes.  The table is launch_octree_build's.
//
//   octree_partition_leaves_kernel  one lane per nonempty leaf: its aligned key and its index as the sort's pair, and 1 to
//                                   histogram[depth] through a histogram of the block's in LDS (22 bins)
//   (rocPRIM radix_sort_pairs)      over the 63 bits of the aligned key: the values are leaf_order, the Leaf_iterator order
//   octree_partition_kernel         ONE wavefront.  The list (key, nrLeafs) lives in LDS.  Per cut: every lane folds split_rank
//                                   over the entries l, l + 64, .. and a 6-step butterfly gives every lane the maximum (the
//                                   index is in the rank: lowest index among equal counts, across chunks too); the threshold;
//                                   lanes 0 .. 7 take one child each (table look-up, nrLeafs by two binary searches), ballot and
//                                   rank order the branch children; the other entries move behind them 64 at a time, from the
//                                   end that keeps a chunk's writes off entries not yet read.  Control flow is wave-uniform
//                                   throughout; the block is the wavefront, so its barrier orders the LDS accesses and no other
//                                   wave is waited for.  On exit: the roots' outputs, the root table the assignment reads, info.
//   octree_partition_assign_kernel  one lane per leaf and per branch: owner_tree walks up the proper ancestors (at most 21
//                                   look-ups in the root table), sub_key re-bases the key
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "launch.h"
#include "octree.hpp"

namespace hpmvs {

__global__ void __launch_bounds__(256) octree_partition_leaves_kernel(const unsigned long long* __restrict__ leaf_key, int nl,
                                                                      unsigned long long* __restrict__ sort_key,
                                                                      int32_t* __restrict__ sort_val, int32_t* __restrict__ histogram) {
    __shared__ int32_t bins[octree::kMaxDepth + 1];
    if (threadIdx.x <= octree::kMaxDepth) bins[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nl) {
        const unsigned long long key = leaf_key[i];
        sort_key[i] = octree::aligned_key(key);
        sort_val[i] = i;
        atomicAdd(&bins[octree::key_depth(key)], 1);   // (the table was checked: 1 .. kMaxDepth)
    }
    __syncthreads();
    if (threadIdx.x <= octree::kMaxDepth && bins[threadIdx.x]) atomicAdd(&histogram[threadIdx.x], bins[threadIdx.x]);
}

__global__ void __launch_bounds__(64) octree_partition_kernel(octree::Cell root, octree::Table t, const unsigned long long* __restrict__ sorted,
                                                              int nl, int min_trees, int min_split_leaves, int cap, OctreePartitionRoots out,
                                                              unsigned long long* root_keys, int32_t* root_vals, uint32_t root_slots,
                                                              int32_t* __restrict__ info) {
#pragma clang fp contract(off)
    __shared__ unsigned long long list_key[octree::kMaxSubtreeList];
    __shared__ int32_t list_count[octree::kMaxSubtreeList];
    const int lane = threadIdx.x;
    const uint64_t* const leaves = (const uint64_t*)sorted;
    int n_trees = 1, n_splits = 0, stop = octree::kStopRoot;
    if (lane == 0) { list_key[0] = octree::kRootKey; list_count[0] = nl; }
    __syncthreads();
    if (min_trees >= 2) {
        uint64_t rank = octree::split_rank(nl, 0);   // "do a first split", whatever the root holds
        while (true) {   // (every cut takes one branch out of the list for good, and n_trees < min_trees <= kMaxSubtrees before one)
            const int m = (int)octree::rank_index(rank);
            const unsigned long long picked = list_key[m];
            uint64_t new_key = 0;
            int32_t new_count = 0;
            const bool branch = lane < 8 && octree::split_child(t, leaves, nl, picked, (unsigned)lane, &new_key, &new_count);
            const unsigned long long mask = __ballot(branch);
            const int n_new = __popcll(mask);
            const int place = __popcll(mask & ((1ull << lane) - 1ull));
            __syncthreads();
            // the other entries: position i -> split_position(i, m, n_new), a chunk read whole before it is written
            if (n_new >= 1) {   // nothing moves down: from the last chunk to the first, a chunk's writes land in it or above it
                for (int lo = ((n_trees - 1) / 64) * 64; lo >= 0; lo -= 64) {
                    const int i = lo + lane;
                    const bool mine = i < n_trees && i != m;
                    const unsigned long long k = mine ? list_key[i] : 0ull;
                    const int32_t c = mine ? list_count[i] : 0;
                    __syncthreads();
                    if (mine) { const int j = octree::split_position(i, m, n_new); list_key[j] = k; list_count[j] = c; }
                    __syncthreads();
                }
            } else {   // the entries behind m move down by one: from m's chunk to the last
                for (int lo = (m / 64) * 64; lo < n_trees; lo += 64) {
                    const int i = lo + lane;
                    const bool mine = i < n_trees && i > m;
                    const unsigned long long k = mine ? list_key[i] : 0ull;
                    const int32_t c = mine ? list_count[i] : 0;
                    __syncthreads();
                    if (mine) { list_key[i - 1] = k; list_count[i - 1] = c; }
                    __syncthreads();
                }
            }
            if (branch) { list_key[place] = new_key; list_count[place] = new_count; }
            __syncthreads();
            n_trees += n_new - 1;
            if (n_trees >= min_trees) { stop = octree::kStopEnough; break; }
            rank = 0;
            for (int i = lane; i < n_trees; i += 64) {
                const uint64_t x = octree::split_rank(list_count[i], (uint32_t)i);
                if (x > rank) rank = x;
            }
            for (int off = 32; off >= 1; off >>= 1) {   // (ranks are distinct: every lane ends with the same one)
                const uint64_t o = __shfl_xor((unsigned long long)rank, off);
                if (o > rank) rank = o;
            }
            if (octree::rank_count(rank) < min_split_leaves) { stop = octree::kStopSmall; break; }
            n_splits++;
        }
    }
    // the roots in list order; entries from n_trees on are 0
    const unsigned long long root_mask = (unsigned long long)root_slots - 1;
    int32_t held = 0;
    for (int lo = 0; lo < cap; lo += 64) {
        const int i = lo + lane;
        if (i >= cap) continue;
        const bool live = i < n_trees;
        const unsigned long long key = live ? list_key[i] : 0ull;
        const int32_t count = live ? list_count[i] : 0;
        held += count;
        if (out.root_key) out.root_key[i] = key;
        if (out.tree_leaves) out.tree_leaves[i] = count;
        if (out.tree_first) out.tree_first[i] = live ? octree::first_leaf(leaves, nl, key) : 0;
        if (out.root_cell) {
            const octree::Cell c = live ? octree::key_cell(root, key) : octree::Cell{{0.0f, 0.0f, 0.0f}, 0.0f};
            out.root_cell[4 * (size_t)i] = c.c[0];
            out.root_cell[4 * (size_t)i + 1] = c.c[1];
            out.root_cell[4 * (size_t)i + 2] = c.c[2];
            out.root_cell[4 * (size_t)i + 3] = c.w;
        }
        if (live) {   // (root_slots > 2 cap: a free slot exists; the keys of the list are distinct)
            unsigned long long h = octree::hash(key) & root_mask;
            while (atomicCAS(&root_keys[h], 0ull, key) != 0ull) h = (h + 1) & root_mask;
            root_vals[h] = i;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) held += __shfl_xor(held, off);
    if (lane == 0) {
        info[kPartitionTrees] = n_trees;
        info[kPartitionOrphans] = nl - held;
        info[kPartitionSplits] = n_splits;
        info[kPartitionStop] = stop;
    }
}

__global__ void __launch_bounds__(256) octree_partition_assign_kernel(const unsigned long long* __restrict__ branch_key, int nb,
                                                                      const unsigned long long* __restrict__ leaf_key, int nl,
                                                                      octree::Table roots, OctreePartitionKeys out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb + nl) return;
    const bool branch = i < nb;
    int32_t* const tree = branch ? out.branch_tree : out.leaf_tree;
    unsigned long long* const sub = branch ? out.branch_sub_key : out.leaf_sub_key;
    if (!tree && !sub) return;
    const int j = branch ? i : i - nb;
    const unsigned long long key = branch ? branch_key[j] : leaf_key[j];
    int root_depth;
    const int32_t owner = octree::owner_tree(roots, key, &root_depth);
    if (tree) tree[j] = owner;
    if (sub) sub[j] = owner < 0 ? 0ull : octree::sub_key(key, root_depth);
}

size_t octree_partition_temp_bytes(int nl) {
    size_t bytes = 0;
    if (nl <= 0) return 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const int32_t*)nullptr,
                                  (int32_t*)nullptr, (size_t)nl, 0u, 63u, (hipStream_t) nullptr) != hipSuccess)
        return (size_t)-1;
    return bytes ? bytes : 1;
}

int launch_octree_partition(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots,
                            const unsigned long long* branch_key, int nb, const unsigned long long* leaf_key, int nl, int min_trees,
                            int min_split_leaves, int cap, const OctreePartitionScratch& s, const OctreePartitionRoots& roots,
                            int32_t* leaf_order, const OctreePartitionKeys& out, hipStream_t st) {
    const octree::Cell r{{root[0], root[1], root[2]}, root[3]};
    const octree::Table t{(const uint64_t*)keys, vals, slots};
    int32_t* const order = leaf_order ? leaf_order : s.val_b;
    if (nl > 0) {
        hipLaunchKernelGGL(octree_partition_leaves_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, leaf_key, nl, s.key_a, s.val_a,
                           s.info + kPartitionHistogram);
        size_t bytes = s.temp_bytes;
        if (rocprim::radix_sort_pairs(s.temp, bytes, (const unsigned long long*)s.key_a, s.key_b, (const int32_t*)s.val_a, order, (size_t)nl, 0u,
                                      63u, st) != hipSuccess)
            return 1;
    }
    hipLaunchKernelGGL(octree_partition_kernel, dim3(1), dim3(64), 0, st, r, t, (const unsigned long long*)s.key_b, nl, min_trees, min_split_leaves,
                       cap, roots, s.root_keys, s.root_vals, s.root_slots, s.info);
    if (nb + nl > 0) {
        const octree::Table rt{(const uint64_t*)s.root_keys, s.root_vals, s.root_slots};
        hipLaunchKernelGGL(octree_partition_assign_kernel, dim3((unsigned)((nb + nl + 255) / 256)), dim3(256), 0, st, branch_key, nb, leaf_key, nl,
                           rt, out);
    }
    return 0;
}

}  // namespace hpmvs
