// Host build of the forest's device block (hpmvs_amd/csrc/octree.hpp: forest_block, forest_block_fill): the layout the three
// forest entry points of capi.hip take from it, checked for one forest and one number of extra header bytes.
// tests/test_cpu_forest_block.py runs it on the forests it names.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared forest_block_host.cpp
// Stand-alone (the same checks on forests it draws itself, some with a doubled key, for a sanitizer run):
//        g++ -std=c++11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -DFOREST_BLOCK_MAIN forest_block_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

// roots: [n_trees][4]; branch_first / leaf_first: [n_trees + 1] (read only for n_trees > 0).  Returns 0, or the line of the check
// that failed.
extern "C" int fb_check(int n_trees, const float* roots, const int32_t* branch_first, const int32_t* leaf_first, const uint64_t* branch_key,
                        const uint64_t* leaf_key, size_t extra_bytes) {
    const size_t T = (size_t)n_trees;
    const ForestBlock b = forest_block(n_trees, branch_first, leaf_first, extra_bytes);
    // every region at a multiple of 256, in the stated order, none reaching into the next; end behind the values
    const size_t at[8] = {b.o_verdict, b.o_trees, b.o_bf, b.o_lf, b.o_extra, b.o_keys, b.o_vals, b.end};
    const size_t size[7] = {sizeof(uint32_t) * kForestWords, sizeof(Tree) * T, 4 * (T + 1), 4 * (T + 1), extra_bytes, 8 * b.slots, 4 * b.slots};
    CHECK(b.o_verdict == 0);
    for (int i = 0; i < 8; i++) CHECK(at[i] % 256 == 0);
    for (int i = 0; i < 7; i++) CHECK(at[i] + size[i] <= at[i + 1]);
    CHECK(b.end >= b.o_vals + 4 * b.slots);
    std::vector<uint64_t> first(T + 1, 0);
    if (n_trees > 0) forest_slots(n_trees, branch_first, leaf_first, first.data());
    CHECK(b.slots == first[T] && b.slot_first == first);
    // the header's image for a block at a made-up device address, over a poisoned buffer
    const uintptr_t base = (uintptr_t)0x7f12345600ull;
    std::vector<char> hdr(b.o_keys, 0x5A);
    forest_block_fill(b, n_trees, roots, branch_first, leaf_first, base, hdr.data());
    for (int v = 0; v < kForestWords; v++) CHECK(((const uint32_t*)hdr.data())[v] == kForestGood);
    const Tree* ht = (const Tree*)(hdr.data() + b.o_trees);
    for (size_t k = 0; k < T; k++) {
        CHECK(memcmp(ht[k].root.c, roots + 4 * k, 12) == 0 && memcmp(&ht[k].root.w, roots + 4 * k + 3, 4) == 0);
        CHECK((uintptr_t)ht[k].t.keys == base + b.o_keys + 8 * first[k] && (uintptr_t)ht[k].t.vals == base + b.o_vals + 4 * first[k]);
        CHECK(ht[k].t.slots == first[k + 1] - first[k]);
    }
    if (n_trees > 0) CHECK(memcmp(hdr.data() + b.o_bf, branch_first, 4 * (T + 1)) == 0 && memcmp(hdr.data() + b.o_lf, leaf_first, 4 * (T + 1)) == 0);
    for (size_t i = 0; i < extra_bytes; i++) CHECK(hdr[b.o_extra + i] == 0);
    // the sequential build over a host block laid out this way: the verdict and the tables of the build over plain vectors, and
    // the trees it points at their slot ranges are the ones the fill made for the block's own address
    std::vector<uint64_t> block(b.end / 8, 0);
    char* w = (char*)block.data();
    forest_block_fill(b, n_trees, roots, branch_first, leaf_first, (uintptr_t)w, w);
    const std::vector<Tree> filled((const Tree*)(w + b.o_trees), (const Tree*)(w + b.o_trees) + T);
    const uint32_t in_block = forest_build_sequential(n_trees, roots, branch_first, leaf_first, branch_key, leaf_key, b.slot_first.data(),
                                                      (uint64_t*)(w + b.o_keys), (int32_t*)(w + b.o_vals), (Tree*)(w + b.o_trees));
    std::vector<uint64_t> keys(first[T], 0);
    std::vector<int32_t> vals(first[T], 0);
    std::vector<Tree> trees(T);
    const uint32_t plain = forest_build_sequential(n_trees, roots, branch_first, leaf_first, branch_key, leaf_key, first.data(), keys.data(),
                                                   vals.data(), trees.data());
    CHECK(in_block == plain);
    for (size_t i = 0; i < keys.size(); i++) CHECK(((const uint64_t*)(w + b.o_keys))[i] == keys[i] && (!keys[i] || ((const int32_t*)(w + b.o_vals))[i] == vals[i]));
    for (size_t k = 0; k < T; k++) {
        const Tree& a = ((const Tree*)(w + b.o_trees))[k];
        CHECK(a.t.keys == filled[k].t.keys && a.t.vals == filled[k].t.vals && a.t.slots == filled[k].t.slots && a.t.slots == trees[k].t.slots);
        CHECK(memcmp(&a.root, &filled[k].root, sizeof(Cell)) == 0);
    }
    return 0;
}

#ifdef FOREST_BLOCK_MAIN
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

int main() {
    int checked = 0;
    for (int round = 0; round < 200; round++) {
        const int T = round < 3 ? round : (int)(rnd() % 140);
        std::vector<float> roots;
        std::vector<int32_t> bf(1, 0), lf(1, 0);
        std::vector<uint64_t> bk, lk;
        for (int k = 0; k < T; k++) {
            const float root[4] = {(float)(rnd() % 100) - 50.0f, (float)(rnd() % 100), 0.5f * (float)k, (float)(1 << (rnd() % 4))};
            roots.insert(roots.end(), root, root + 4);
            // distinct leaves at depth 2 and the depth-1 branches above them; every seventh round doubles a leaf of the middle tree
            bool leaf[64] = {false}, branch[8] = {false};
            const int want = k % 3 == 1 ? 0 : (int)(rnd() % 33);
            for (int j = 0; j < want; j++) leaf[rnd() % 64] = true;
            for (int j = 0; j < 64; j++)
                if (leaf[j]) { lk.push_back((uint64_t)(0100 | j)); branch[j >> 3] = true; }
            for (int j = 0; j < 8; j++)
                if (branch[j]) bk.push_back((uint64_t)(010 | j));
            if (round % 7 == 6 && k == T / 2 && (int32_t)lk.size() > lf.back()) lk.push_back(lk.back());
            bf.push_back((int32_t)bk.size());
            lf.push_back((int32_t)lk.size());
        }
        for (size_t extra : {(size_t)0, (size_t)T}) {
            const int line = fb_check(T, roots.data(), bf.data(), lf.data(), bk.data(), lk.data(), extra);
            if (line) { std::printf("round %d, %d trees, %zu extra bytes: the check at line %d failed\n", round, T, extra, line); return 1; }
            checked++;
        }
    }
    std::printf("forest_block_host: %d blocks laid out, filled and built\n", checked);
    return 0;
}
#endif
