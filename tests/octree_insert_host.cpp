// Host restatement of hpmvs_octree_insert_batch and hpmvs_octree_route_batch (include/hpmvs_amd.h): the product's rules
// (hpmvs_amd/csrc/octree.hpp: insert_sequential, contains) compiled by g++, with a sequential table build in place of the
// device's compare-and-swap.  tests/test_cpu_octree_insert.py pins it to a loop of addConditional on the pointer tree; the GPU
// tests compare the kernels with it byte for byte.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared octree_insert_host.cpp
#include <cstdint>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

// root: c_ (3), width_.  Outputs as hpmvs_octree_insert_batch (blocker nullable).  Returns 0, or -2 for keys that are no tree
// (nothing written).
int ot_insert(const float* root, int nb, const uint64_t* branch_key, int nl, const uint64_t* leaf_key, int n, const float* points,
              const float* add_width, uint8_t* accepted, uint64_t* out_key, int32_t* blocker) {
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
    const Cell r{{root[0], root[1], root[2]}, root[3]};
    insert_sequential(r, t, n, points, add_width, accepted, out_key, blocker);
    return 0;
}

// roots: [n_trees][4].  tree[i]: the first root in list order that contains points[i], -1 when none does.
void ot_route(int n_trees, const float* roots, int n, const float* points, int32_t* tree) {
    for (int i = 0; i < n; i++) {
        tree[i] = -1;
        for (int t = 0; t < n_trees && tree[i] < 0; t++) {
            const Cell r{{roots[4 * t], roots[4 * t + 1], roots[4 * t + 2]}, roots[4 * t + 3]};
            if (contains(r, points + 3 * (size_t)i)) tree[i] = t;
        }
    }
}

}  // extern "C"
