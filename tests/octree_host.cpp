// Host restatement of hpmvs_octree_locate_batch (include/hpmvs_amd.h): the product's rules (hpmvs_amd/csrc/octree.hpp) compiled
// by g++, with a sequential table build in place of the device's compare-and-swap.  tests/test_cpu_octree_index.py pins it to the
// pointer tree of tests/octree_tree_ref.py; the GPU tests compare the kernels with it byte for byte.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared octree_host.cpp
#include <cstdint>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

// root: c_ (3), width_.  Outputs as hpmvs_octree_locate_batch, each nullable.  Returns 0, or -2 for keys that are no tree (nothing
// written; *verdict, nullable, receives the kBad* bits).
int ot_locate(const float* root, int nb, const uint64_t* branch_key, int nl, const uint64_t* leaf_key, int n, const float* points,
              const float* add_width, uint8_t* inside, uint64_t* out_key, int32_t* out_index, float* out_width, float* out_center,
              uint64_t* target_key, int32_t* verdict) {
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
    if (verdict) *verdict = bad;
    if (bad) return -2;
    const Cell r{{root[0], root[1], root[2]}, root[3]};
    for (int i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        const Located l = locate(r, t, p);
        if (inside) inside[i] = contains(r, p) ? 1 : 0;
        if (out_key) out_key[i] = l.key;
        if (out_index) out_index[i] = l.index;
        if (out_width) out_width[i] = l.cell.w;
        if (out_center)
            for (int k = 0; k < 3; k++) out_center[3 * (size_t)i + k] = l.cell.c[k];
        if (target_key) target_key[i] = add_width ? add_target(l, p, add_width[i]) : 0;
    }
    return 0;
}

}  // extern "C"
