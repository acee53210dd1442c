// Host build of hpmvs_border_forest_batch (include/hpmvs_amd.h): hpmvs_amd/csrc/octree.hpp's border_forest_sequential -- the
// route loop, then insert_sequential per tree over that tree's rows -- over the tables forest_build_sequential makes, compiled by
// g++.  tests/test_cpu_border_forest.py pins it to ot_route and per-tree ot_insert (tests/octree_insert_host.cpp) composed in
// Python; the GPU tests compare the one call with it byte for byte.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared border_forest_host.cpp
#include <cstdint>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

constexpr int kFoundOffsets = 8;   // beside kBadKey / kBadTwice / kBadOrphan

// roots: [n_trees][4]; center: [n][4], scale: [n] as a patch batch holds them.  Outputs as hpmvs_border_forest_result (blocker
// nullable).  Returns 0, or -2 with nothing written but found[0] = what and found[1] = the lowest offending tree.
int bf_border(int n_trees, const float* roots, const int32_t* branch_first, const int32_t* leaf_first, const uint64_t* branch_key,
              const uint64_t* leaf_key, int n, const float* center, const float* scale, int32_t* tree, uint8_t* accepted, uint64_t* out_key,
              int32_t* blocker, int32_t* found) {
    found[0] = found[1] = 0;
    std::vector<Tree> trees((size_t)n_trees);
    std::vector<uint64_t> keys;
    std::vector<int32_t> vals;
    if (n_trees > 0) {
        int32_t bad = forest_offsets_bad(n_trees, branch_first);
        if (bad < 0) bad = forest_offsets_bad(n_trees, leaf_first);
        if (bad >= 0) { found[0] = kFoundOffsets; found[1] = bad; return -2; }
        std::vector<uint64_t> slot_first((size_t)n_trees + 1);
        forest_slots(n_trees, branch_first, leaf_first, slot_first.data());
        keys.assign(slot_first[n_trees], 0);
        vals.assign(slot_first[n_trees], 0);
        const uint32_t verdict = forest_build_sequential(n_trees, roots, branch_first, leaf_first, branch_key, leaf_key, slot_first.data(),
                                                         keys.data(), vals.data(), trees.data());
        if (verdict != kForestGood) { found[0] = finding_bad(verdict); found[1] = finding_tree(verdict); return -2; }
    }
    border_forest_sequential(n_trees, trees.data(), n, center, scale, tree, accepted, out_key, blocker);
    return 0;
}

}  // extern "C"
