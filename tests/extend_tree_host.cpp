// Host build of the extend level's two look-ups (hpmvs_amd/csrc/octree.hpp: extend_pre, extend_post, level_depth, extend_add_width)
// as the kernels of kernel_extend_tree.hip apply them, with a sequential table build in place of the device's compare-and-swap.
// tests/test_cpu_extend_tree.py pins it to the pointer tree of tests/octree_tree_ref.py.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared extend_tree_host.cpp
#include <cstdint>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

int et_level_depth(float root_width, float width) { return level_depth(root_width, width); }
float et_add_width(float width) { return extend_add_width(width); }

// root: c_ (3), width_.  Every point is taken both as a centre before optimize (skip, pre_inside, pre_key) and as a refined one
// (border, post_key).  Returns 0, or -2 for keys that are no tree or a width that is no level width (nothing written).
int et_extend(const float* root, int nb, const uint64_t* branch_key, int nl, const uint64_t* leaf_key, int n, const float* points,
              float width, uint8_t* skip, uint8_t* pre_inside, uint64_t* pre_key, uint8_t* border, uint64_t* post_key) {
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
    if (bad || level_depth(root[3], width) < 0) return -2;
    const Cell r{{root[0], root[1], root[2]}, root[3]};
    const float aw = extend_add_width(width);
    for (int i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        const ExtendPre a = extend_pre(r, t, p, width, aw);
        const ExtendPost b = extend_post(r, t, p, aw);
        skip[i] = a.skip ? 1 : 0;
        pre_inside[i] = a.inside ? 1 : 0;
        pre_key[i] = a.pre_key;
        border[i] = b.border ? 1 : 0;
        post_key[i] = b.post_key;
    }
    return 0;
}

}  // extern "C"
