// insert_sequential (hpmvs_amd/csrc/octree.hpp) on a generated tree, checked by its invariants; a stand-alone program meant for
// the sanitizers.  It is not loaded into Python and uses no GPU.
//   g++ -std=c++11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all octree_insert_selftest.cpp -o octree_insert_selftest
//   ./octree_insert_selftest
// The tree: random points split a cube down to random widths (the branches are their paths' prefixes, every eighth leaf is left
// empty).  The patches: inside, outside and non-finite points, widths over sixteen octaves and 0, negative, NaN, inf; half of
// them aimed at a few empty leaves so that the runs grow long.  Checked: no accepted key is a prefix of (or equal to) another or
// of a leaf of the tree, or lies on a branch; every accepted key's proper prefixes are absent from the leaf set; a refusal names
// a blocker that was accepted earlier, and its leaf lies under the same static leaf.
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
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const Cell root{{0.5f, -1.0f, 2.0f}, 7.0f};
    std::set<uint64_t> branches, leaves;
    for (int i = 0; i < 4000; i++) {
        const float p[3] = {root.c[0] + (U(rng) - 0.5f) * root.w, root.c[1] + (U(rng) - 0.5f) * root.w, root.c[2] + (U(rng) - 0.5f) * root.w};
        const uint64_t path = full_path(root, p);
        const int depth = 2 + (int)(U(rng) * 9);
        uint64_t k = path_prefix(path, depth);
        bool below = false;   // a leaf may not sit on or under another one, nor on a branch
        for (int d = 1; d <= depth; d++) below = below || leaves.count(path_prefix(path, d));
        if (below || branches.count(k)) continue;
        if (i % 8) leaves.insert(k);
        for (k >>= 3; k > 1; k >>= 3) branches.insert(k);
    }
    for (auto it = leaves.begin(); it != leaves.end();) it = branches.count(*it) ? leaves.erase(it) : ++it;
    const std::vector<uint64_t> bk(branches.begin(), branches.end()), lk(leaves.begin(), leaves.end());
    const uint32_t slots = table_slots(bk.size() + lk.size());
    std::vector<uint64_t> keys(slots, 0);
    std::vector<int32_t> vals(slots, 0);
    for (size_t i = 0; i < bk.size(); i++) CHECK(!key_form(bk[i], true) && insert(keys.data(), vals.data(), slots, bk[i], kBranch));
    for (size_t i = 0; i < lk.size(); i++) CHECK(!key_form(lk[i], false) && insert(keys.data(), vals.data(), slots, lk[i], (int32_t)i));
    const Table t{keys.data(), vals.data(), slots};
    for (uint64_t k : bk) CHECK(!key_parentage(t, k));
    for (uint64_t k : lk) CHECK(!key_parentage(t, k));

    const int n = 20000;
    std::vector<float> pts(3 * (size_t)n), aw(n);
    float hot[8][3];
    for (auto& h : hot)
        for (int k = 0; k < 3; k++) h[k] = root.c[k] + (U(rng) - 0.5f) * root.w;
    const float odd[6] = {0.0f, -1.0f, std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 1e-30f};
    for (int i = 0; i < n; i++) {
        float* p = &pts[3 * (size_t)i];
        const float spread = i % 2 ? 1.6f : 0.02f;   // (1.6: a fifth of the points lie outside the root)
        const float* c = i % 2 ? root.c : hot[(i / 2) % 8];
        for (int k = 0; k < 3; k++) p[k] = c[k] + (U(rng) - 0.5f) * root.w * spread;
        if (i % 97 == 0) p[i % 3] = odd[2 + (i / 97) % 3];
        aw[i] = i % 41 == 0 ? odd[(i / 41) % 6] : root.w * std::exp2(-16.0f * U(rng));
    }
    std::vector<uint8_t> accepted(n, 7);
    std::vector<uint64_t> leaf_key(n, 0);
    std::vector<int32_t> blocker(n, 7);
    insert_sequential(root, t, n, pts.data(), aw.data(), accepted.data(), leaf_key.data(), blocker.data());
    std::vector<uint64_t> leaf_only(n, 0);
    std::vector<uint8_t> acc_only(n, 7);
    insert_sequential(root, t, n, pts.data(), aw.data(), acc_only.data(), leaf_only.data(), nullptr);
    CHECK(acc_only == accepted && leaf_only == leaf_key);

    std::set<uint64_t> now(leaves);
    int n_acc = 0, n_dyn = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t k = leaf_key[i];
        const int d = key_depth(k);
        CHECK(accepted[i] <= 1 && d >= 1 && d <= kMaxDepth);
        CHECK(path_prefix(full_path(root, &pts[3 * (size_t)i]), d) == k);   // the leaf lies on the point's path
        if (accepted[i]) {
            n_acc++;
            CHECK(blocker[i] == -1 && !branches.count(k));
            CHECK(now.insert(k).second);   // not equal to a leaf of the tree or to an earlier accepted key
        } else if (blocker[i] >= 0) {
            n_dyn++;
            CHECK(blocker[i] < i && accepted[blocker[i]]);
            const Located a = locate(root, t, &pts[3 * (size_t)i]), b = locate(root, t, &pts[3 * (size_t)blocker[i]]);
            CHECK(a.key == b.key && a.index == kAbsent);
        } else {
            CHECK(blocker[i] == -1);
            const Located a = locate(root, t, &pts[3 * (size_t)i]);
            CHECK(a.key == k && (a.index != kAbsent || a.cell.w < aw[i]));
        }
    }
    for (uint64_t k : now)   // prefix-free: no key below or above another, every parent absent from the leaf set
        for (uint64_t q = k >> 3; q >= 1; q >>= 3) CHECK(!now.count(q));
    printf("octree_insert_selftest: %zu branches, %zu leaves, %d patches: %d accepted, %d refused by an earlier patch, %d failures\n",
           bk.size(), lk.size(), n, n_acc, n_dyn, failures);
    CHECK(n_acc > 1000 && n_dyn > 1000);
    return failures ? 1 : 0;
}
