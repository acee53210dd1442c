// Host restatement of hpmvs_octree_partition (include/hpmvs_amd.h): the product's rules (hpmvs_amd/csrc/octree.hpp:
// partition_sequential, nr_leafs, key_cell, owner_tree, sub_key) compiled by g++, with a sequential table build and std::sort in
// place of the device's compare-and-swap and radix sort.  tests/test_cpu_octree_partition.py pins it to the loop of main's
// getSubTrees on the pointer tree; the GPU tests compare the kernels with it byte for byte.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared octree_partition_host.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

// root: c_ (3), width_.  info: n_trees, n_orphans, n_splits, stop, histogram[22].  Outputs as hpmvs_octree_partition, every one
// nullable; the roots' hold max(8, min_trees + 6) entries.  Returns 0, or -2 for what the call refuses (nothing written).
int ot_partition(const float* root, int nb, const uint64_t* branch_key, int nl, const uint64_t* leaf_key, int min_trees,
                 int min_split_leaves, int32_t* info, uint64_t* root_key, float* root_cell, int32_t* tree_first, int32_t* tree_leaves,
                 int32_t* leaf_order, int32_t* leaf_tree, uint64_t* leaf_sub_key, int32_t* branch_tree, uint64_t* branch_sub_key) {
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(root[k])) return -2;
    if (!(root[3] > 0.0f) || min_trees > kMaxSubtrees || min_split_leaves < 1) return -2;
    const uint32_t slots = table_slots((size_t)nb + (size_t)nl);
    std::vector<uint64_t> keys(slots, 0);
    std::vector<int32_t> vals(slots, 0);
    int bad = 0;
    for (int i = 0; i < nb + nl; i++) {
        const bool branch = i < nb;
        const uint64_t key = branch ? branch_key[i] : leaf_key[i - nb];
        const int form = key_form(key, branch);
        if (form) { bad |= form; continue; }
        if (!insert(keys.data(), vals.data(), slots, key, branch ? kBranch : i - nb)) bad |= kBadTwice;
    }
    const Table t{keys.data(), vals.data(), slots};
    for (int i = 0; i < nb + nl; i++) {
        const uint64_t key = i < nb ? branch_key[i] : leaf_key[i - nb];
        if (!key_form(key, i < nb)) bad |= key_parentage(t, key);
    }
    if (bad) return -2;

    // Leaf_iterator order and cellHistogram
    std::vector<std::pair<uint64_t, int32_t> > order((size_t)nl);
    for (int i = 0; i < 4 + kMaxDepth + 1; i++) info[i] = 0;
    for (int i = 0; i < nl; i++) {
        order[i] = std::make_pair(aligned_key(leaf_key[i]), (int32_t)i);
        info[4 + key_depth(leaf_key[i])]++;
    }
    std::sort(order.begin(), order.end());
    std::vector<uint64_t> sorted((size_t)nl);
    for (int i = 0; i < nl; i++) {
        sorted[i] = order[i].first;
        if (leaf_order) leaf_order[i] = order[i].second;
    }

    const int cap = min_trees + 6 > 8 ? min_trees + 6 : 8;
    std::vector<uint64_t> list_key((size_t)cap, 0);
    std::vector<int32_t> list_count((size_t)cap, 0);
    const Split r = partition_sequential(t, sorted.data(), nl, min_trees, min_split_leaves, list_key.data(), list_count.data());

    const Cell rc{{root[0], root[1], root[2]}, root[3]};
    const uint32_t root_slots = table_slots((size_t)cap);
    std::vector<uint64_t> rk(root_slots, 0);
    std::vector<int32_t> rv(root_slots, 0);
    int32_t held = 0;
    for (int i = 0; i < cap; i++) {
        const bool live = i < r.n_trees;
        const uint64_t key = live ? list_key[i] : 0;
        const int32_t count = live ? list_count[i] : 0;
        held += count;
        if (root_key) root_key[i] = key;
        if (tree_leaves) tree_leaves[i] = count;
        if (tree_first) tree_first[i] = live ? first_leaf(sorted.data(), nl, key) : 0;
        if (root_cell) {
            const Cell c = live ? key_cell(rc, key) : Cell{{0.0f, 0.0f, 0.0f}, 0.0f};
            for (int k = 0; k < 3; k++) root_cell[4 * i + k] = c.c[k];
            root_cell[4 * i + 3] = c.w;
        }
        if (live) insert(rk.data(), rv.data(), root_slots, key, i);
    }
    info[0] = r.n_trees;
    info[1] = nl - held;
    info[2] = r.n_splits;
    info[3] = r.stop;

    const Table roots{rk.data(), rv.data(), root_slots};
    for (int i = 0; i < nb + nl; i++) {
        const bool branch = i < nb;
        const int j = branch ? i : i - nb;
        const uint64_t key = branch ? branch_key[j] : leaf_key[j];
        int32_t* const tree = branch ? branch_tree : leaf_tree;
        uint64_t* const sub = branch ? branch_sub_key : leaf_sub_key;
        int root_depth;
        const int32_t owner = owner_tree(roots, key, &root_depth);
        if (tree) tree[j] = owner;
        if (sub) sub[j] = owner < 0 ? 0 : sub_key(key, root_depth);
    }
    return 0;
}

}  // extern "C"
