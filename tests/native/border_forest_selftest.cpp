// border_forest_sequential (hpmvs_amd/csrc/octree.hpp) on a generated forest, checked by its invariants; a stand-alone program
// meant for the sanitizers.  It is not loaded into Python and uses no GPU.
//   g++ -std=c++11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all border_forest_selftest.cpp -o border_forest_selftest
//   ./border_forest_selftest
// The forest: five trees side by side, three root widths, one without keys, two with the SAME key sets (random points split a
// cube down to random widths; every eighth leaf is left empty).  The queue: 20 000 patches whose rows interleave the trees,
// inside, between and outside the roots and non-finite, scales over sixteen octaves and 0, negative, NaN, inf; half of them aimed
// at a few spots so that the runs grow long.  Checked: tree[] is the first root that contains the point; per tree no accepted
// key is a prefix of (or equal to) another or of a leaf of the tree, or lies on a branch; a refusal names a blocker that was
// accepted earlier IN THE SAME TREE under the same static leaf; an unrouted row has no key and no blocker.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "../../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    std::mt19937 rng(54321);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const int T = 5;
    const float roots[T][4] = {{0.5f, -1.0f, 2.0f, 7.0f}, {10.0f, 0.0f, 0.0f, 3.5f}, {20.0f, 1.0f, -1.0f, 14.0f}, {40.0f, 0.0f, 0.0f, 7.0f},
                               {47.0f, 0.0f, 0.0f, 7.0f}};   // (trees 3 and 4 share a face)
    std::set<uint64_t> branches[T], leaves[T];
    for (int k = 0; k < T; k++) {
        if (k == 1) continue;                                        // a tree without keys
        if (k == 4) { branches[4] = branches[0]; leaves[4] = leaves[0]; continue; }   // the same sub-keys under another root
        const Cell root{{roots[k][0], roots[k][1], roots[k][2]}, roots[k][3]};
        for (int i = 0; i < 1500; i++) {
            const float p[3] = {root.c[0] + (U(rng) - 0.5f) * root.w, root.c[1] + (U(rng) - 0.5f) * root.w, root.c[2] + (U(rng) - 0.5f) * root.w};
            const uint64_t path = full_path(root, p);
            const int depth = 2 + (int)(U(rng) * 8);
            uint64_t key = path_prefix(path, depth);
            bool below = false;   // a leaf may not sit on or under another one, nor on a branch
            for (int d = 1; d <= depth; d++) below = below || leaves[k].count(path_prefix(path, d));
            if (below || branches[k].count(key)) continue;
            if (i % 8) leaves[k].insert(key);
            for (key >>= 3; key > 1; key >>= 3) branches[k].insert(key);
        }
        for (auto it = leaves[k].begin(); it != leaves[k].end();) it = branches[k].count(*it) ? leaves[k].erase(it) : ++it;
    }
    std::vector<uint64_t> bk, lk;
    std::vector<int32_t> bf(1, 0), lf(1, 0);
    for (int k = 0; k < T; k++) {
        bk.insert(bk.end(), branches[k].begin(), branches[k].end());
        lk.insert(lk.end(), leaves[k].begin(), leaves[k].end());
        bf.push_back((int32_t)bk.size());
        lf.push_back((int32_t)lk.size());
    }
    std::vector<uint64_t> slot_first(T + 1);
    forest_slots(T, bf.data(), lf.data(), slot_first.data());
    std::vector<uint64_t> keys(slot_first[T], 0);
    std::vector<int32_t> vals(slot_first[T], 0);
    std::vector<Tree> trees(T);
    CHECK(forest_build_sequential(T, &roots[0][0], bf.data(), lf.data(), bk.data(), lk.data(), slot_first.data(), keys.data(), vals.data(),
                                  trees.data()) == kForestGood);

    const int n = 20000;
    std::vector<float> center(4 * (size_t)n, 1.0f), scale(n);
    float hot[10][3];
    for (int h = 0; h < 10; h++)
        for (int c = 0; c < 3; c++) hot[h][c] = roots[h % T][c] + (U(rng) - 0.5f) * roots[h % T][3];
    const float odd[6] = {0.0f, -1.0f, std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 1e-30f};
    for (int i = 0; i < n; i++) {
        float* p = &center[4 * (size_t)i];
        const int k = (int)(rng() % T);
        const float spread = i % 2 ? 1.6f : 0.02f;   // (1.6: a fifth of the points lie outside their root)
        const float* c = i % 2 ? roots[k] : hot[(i / 2) % 10];
        const float w = i % 2 ? roots[k][3] : 7.0f;
        for (int j = 0; j < 3; j++) p[j] = c[j] + (U(rng) - 0.5f) * w * spread;
        if (i % 97 == 0) p[i % 3] = odd[2 + (i / 97) % 3];
        scale[i] = i % 41 == 0 ? odd[(i / 41) % 6] : 7.0f * std::exp2(-16.0f * U(rng));
    }
    std::vector<int32_t> tree(n, 7), blocker(n, 7);
    std::vector<uint8_t> accepted(n, 7);
    std::vector<uint64_t> leaf_key(n, 7);
    border_forest_sequential(T, trees.data(), n, center.data(), scale.data(), tree.data(), accepted.data(), leaf_key.data(), blocker.data());
    std::vector<int32_t> tree_only(n, 7);
    std::vector<uint8_t> acc_only(n, 7);
    std::vector<uint64_t> leaf_only(n, 7);
    border_forest_sequential(T, trees.data(), n, center.data(), scale.data(), tree_only.data(), acc_only.data(), leaf_only.data(), nullptr);
    CHECK(tree_only == tree && acc_only == accepted && leaf_only == leaf_key);

    std::set<uint64_t> now[T];
    for (int k = 0; k < T; k++) now[k] = leaves[k];
    int n_acc = 0, n_dyn = 0, n_out = 0, reached[T] = {0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        const float* p = &center[4 * (size_t)i];
        int first = -1;
        for (int k = T - 1; k >= 0; k--)
            if (contains(trees[k].root, p)) first = k;
        CHECK(tree[i] == first);
        if (first < 0) {
            n_out++;
            CHECK(accepted[i] == 0 && leaf_key[i] == 0 && blocker[i] == -1);
            continue;
        }
        const Tree& tr = trees[first];
        reached[first]++;
        const uint64_t key = leaf_key[i];
        const int d = key_depth(key);
        CHECK(accepted[i] <= 1 && d >= 1 && d <= kMaxDepth);
        CHECK(path_prefix(full_path(tr.root, p), d) == key);   // the leaf lies on the point's path in ITS tree
        if (accepted[i]) {
            n_acc++;
            CHECK(blocker[i] == -1 && !branches[first].count(key));
            CHECK(now[first].insert(key).second);   // not equal to a leaf of the tree or to an earlier accepted key of the tree
        } else if (blocker[i] >= 0) {
            n_dyn++;
            CHECK(blocker[i] < i && accepted[blocker[i]] && tree[blocker[i]] == first);
            const Located a = locate(tr.root, tr.t, p), b = locate(tr.root, tr.t, &center[4 * (size_t)blocker[i]]);
            CHECK(a.key == b.key && a.index == kAbsent);
        } else {
            CHECK(blocker[i] == -1);
            const Located a = locate(tr.root, tr.t, p);
            CHECK(a.key == key && (a.index != kAbsent || a.cell.w < border_add_width(scale[i])));
        }
    }
    for (int k = 0; k < T; k++)   // prefix-free per tree: no key below or above another
        for (uint64_t key : now[k])
            for (uint64_t q = key >> 3; q >= 1; q >>= 3) CHECK(!now[k].count(q));
    printf("border_forest_selftest: %zu branches, %zu leaves in %d trees, %d patches (%d %d %d %d %d per tree, %d unrouted): %d accepted, "
           "%d refused by an earlier patch, %d failures\n", bk.size(), lk.size(), T, n, reached[0], reached[1], reached[2], reached[3],
           reached[4], n_out, n_acc, n_dyn, failures);
    CHECK(n_acc > 1000 && n_dyn > 1000 && n_out > 500);
    for (int k = 0; k < T; k++) CHECK(reached[k] > 500);
    return failures ? 1 : 0;
}
