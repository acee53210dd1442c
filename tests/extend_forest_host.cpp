// Host build of the forest form of the extend level's look-ups (hpmvs_amd/csrc/octree.hpp: forest_slots, forest_offsets_bad,
// tree_of, forest_key, forest_build_sequential, forest_check_key, extend_forest_pre / extend_forest_post) as the kernels of
// kernel_extend_forest.hip apply them, with the sequential build in place of the device's compare-and-swap.
// tests/test_cpu_extend_forest.py pins it to the per-tree functions (tests/extend_tree_host.cpp) on random forests.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared extend_forest_host.cpp
// Stand-alone (a self-check of the same comparison on forests it draws itself, for a sanitizer run):
//        g++ -std=c++11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -DEXTEND_FOREST_MAIN extend_forest_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

constexpr int kFoundOffsets = 8, kFoundParent = 16, kFoundLevel = 32;   // beside kBadKey / kBadTwice / kBadOrphan

// slot_first: [n_trees + 1]
void ef_slots(int n_trees, const int32_t* branch_first, const int32_t* leaf_first, uint64_t* slot_first) {
    forest_slots(n_trees, branch_first, leaf_first, slot_first);
}
int ef_tree_of(const int32_t* first, int n_trees, int i) { return tree_of(first, n_trees, i); }

// roots: [n_trees][4].  Point i belongs to tree point_tree[i] and is taken both as a centre before optimize and as a refined
// one, as et_extend takes it.  Returns 0, or -2 with nothing written but found[0] = what (one of the constants above, or a kBad*
// bit) and found[1] = the offending tree (for kFoundParent: the point).
int ef_extend(int n_trees, const float* roots, const int32_t* branch_first, const int32_t* leaf_first, const uint64_t* branch_key,
              const uint64_t* leaf_key, int n, const float* points, const int32_t* point_tree, float width, uint8_t* skip,
              uint8_t* pre_inside, uint64_t* pre_key, uint8_t* border, uint64_t* post_key, int32_t* found) {
    found[0] = found[1] = 0;
    if (n_trees == 0) return n == 0 ? 0 : (found[0] = kFoundParent, found[1] = 0, -2);
    int32_t bad = forest_offsets_bad(n_trees, branch_first);
    if (bad < 0) bad = forest_offsets_bad(n_trees, leaf_first);
    if (bad >= 0) { found[0] = kFoundOffsets; found[1] = bad; return -2; }
    std::vector<uint64_t> slot_first((size_t)n_trees + 1);
    forest_slots(n_trees, branch_first, leaf_first, slot_first.data());
    std::vector<uint64_t> keys(slot_first[n_trees], 0);
    std::vector<int32_t> vals(slot_first[n_trees], 0);
    std::vector<Tree> trees(n_trees);
    const uint32_t verdict = forest_build_sequential(n_trees, roots, branch_first, leaf_first, branch_key, leaf_key, slot_first.data(),
                                                     keys.data(), vals.data(), trees.data());
    if (verdict != kForestGood) { found[0] = finding_bad(verdict); found[1] = finding_tree(verdict); return -2; }
    uint32_t parent = kForestGood, level = kForestGood;   // the parents kernel: both folded with min
    for (int i = 0; i < n; i++) {
        const int32_t k = point_tree[i];
        if (k < 0 || k >= n_trees) { if ((uint32_t)i < parent) parent = (uint32_t)i; }
        else if (level_depth(trees[k].root.w, width) < 0 && (uint32_t)k < level) level = (uint32_t)k;
    }
    if (parent != kForestGood) { found[0] = kFoundParent; found[1] = (int32_t)parent; return -2; }
    if (level != kForestGood) { found[0] = kFoundLevel; found[1] = (int32_t)level; return -2; }
    const float aw = extend_add_width(width);
    for (int i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        const ExtendPre a = extend_forest_pre(trees.data(), point_tree[i], p, width, aw);
        const ExtendPost b = extend_forest_post(trees.data(), point_tree[i], p, aw);
        skip[i] = a.skip ? 1 : 0;
        pre_inside[i] = a.inside ? 1 : 0;
        pre_key[i] = a.pre_key;
        border[i] = b.border ? 1 : 0;
        post_key[i] = b.post_key;
    }
    return 0;
}

}  // extern "C"

#ifdef EXTEND_FOREST_MAIN
// The per-tree functions on one tree's own table, as tests/extend_tree_host.cpp has them.
static int one_tree(const float* root, int nb, const uint64_t* bk, int nl, const uint64_t* lk, int n, const float* points, float width,
                    uint8_t* skip, uint8_t* pre_inside, uint64_t* pre_key, uint8_t* border, uint64_t* post_key) {
    const uint32_t slots = table_slots((size_t)nb + (size_t)nl);
    std::vector<uint64_t> keys(slots, 0);
    std::vector<int32_t> vals(slots, 0);
    int bad = 0;
    for (int i = 0; i < nb + nl; i++) {
        const uint64_t key = i < nb ? bk[i] : lk[i - nb];
        const int form = key_form(key, i < nb);
        if (form) { bad |= form; continue; }
        if (!insert(keys.data(), vals.data(), slots, key, i < nb ? kBranch : i - nb)) bad |= kBadTwice;
    }
    const Table t{keys.data(), vals.data(), slots};
    for (int i = 0; i < nb + nl; i++) {
        const uint64_t key = i < nb ? bk[i] : lk[i - nb];
        if (!key_form(key, i < nb)) bad |= key_parentage(t, key);
    }
    if (bad || level_depth(root[3], width) < 0) return -2;
    const Cell r{{root[0], root[1], root[2]}, root[3]};
    const float aw = extend_add_width(width);
    for (int i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        const ExtendPre a = extend_pre(r, t, p, width, aw);
        const ExtendPost b = extend_post(r, t, p, aw);
        skip[i] = a.skip; pre_inside[i] = a.inside; pre_key[i] = a.pre_key; border[i] = b.border; post_key[i] = b.post_key;
    }
    return 0;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }
static float unit() { return (float)(rnd() % 100001) / 100000.0f - 0.5f; }

int main() {
    int compared = 0, refused = 0;
    for (int round = 0; round < 300; round++) {
        const int T = (int)(rnd() % 7);
        std::vector<float> roots;
        std::vector<int32_t> bf(1, 0), lf(1, 0);
        std::vector<uint64_t> bk, lk;
        for (int k = 0; k < T; k++) {
            const float W = 4.0f * (float)(1 << (rnd() % 2));
            const float root[4] = {unit(), unit(), unit(), W};
            roots.insert(roots.end(), root, root + 4);
            // a tree by insertion: random leaf keys of depth 1 .. 6, kept prefix-free; every proper prefix becomes a branch
            std::vector<uint64_t> tb, tl;
            const int want = k == 1 ? 0 : k == 2 ? 1 : (int)(rnd() % 40);
            for (int j = 0; j < want; j++) {
                const int d = 1 + (int)(rnd() % 6);
                uint64_t key = 1;
                for (int l = 0; l < d; l++) key = (key << 3) | (rnd() & 7u);
                bool clash = false;
                for (uint64_t o : tl) {
                    const int od = key_depth(o), m = od < d ? od : d;
                    if ((o >> (3 * (od - m))) == (key >> (3 * (d - m)))) clash = true;
                }
                for (uint64_t o : tb) if (o == key) clash = true;
                if (clash) continue;
                tl.push_back(key);
                for (uint64_t a = key >> 3; a > 1; a >>= 3) {
                    bool have = false;
                    for (uint64_t o : tb) if (o == a) have = true;
                    if (!have) tb.push_back(a);
                }
            }
            if (round % 5 == 4 && k == T / 2 && !tl.empty()) {   // a bad middle tree
                const int kind = (round / 5) % 3;
                if (kind == 0) tl.push_back(2);
                else if (kind == 1) tl.push_back(tl[0]);
                else tl.push_back((tl[0] << 6) | 011);
            }
            bk.insert(bk.end(), tb.begin(), tb.end());
            lk.insert(lk.end(), tl.begin(), tl.end());
            bf.push_back((int32_t)bk.size());
            lf.push_back((int32_t)lk.size());
        }
        const float width = 0.5f;
        const int n = T ? 64 : 0;
        std::vector<float> pts(3 * (size_t)n);
        std::vector<int32_t> pt(n);
        for (int i = 0; i < n; i++) {
            pt[i] = (int32_t)(rnd() % (uint32_t)T);
            for (int c = 0; c < 3; c++) pts[3 * i + c] = roots[4 * pt[i] + c] + unit() * roots[4 * pt[i] + 3] * 1.2f;
        }
        std::vector<uint8_t> skip(n, 0x5A), inside(n, 0x5A), border(n, 0x5A);
        std::vector<uint64_t> pre(n, 0x5A5A), post(n, 0x5A5A);
        int32_t found[2];
        const int rc = ef_extend(T, roots.data(), bf.data(), lf.data(), bk.data(), lk.data(), n, pts.data(), pt.data(), width, skip.data(),
                                 inside.data(), pre.data(), border.data(), post.data(), found);
        int first_bad = -1;
        for (int k = 0; k < T; k++) {
            std::vector<float> p;
            std::vector<int> at;
            for (int i = 0; i < n; i++)
                if (pt[i] == k) { p.insert(p.end(), &pts[3 * i], &pts[3 * i] + 3); at.push_back(i); }
            const int m = (int)at.size();
            std::vector<uint8_t> s(m), in(m), bo(m);
            std::vector<uint64_t> pr(m), po(m);
            const int one = one_tree(&roots[4 * k], bf[k + 1] - bf[k], bk.data() + bf[k], lf[k + 1] - lf[k], lk.data() + lf[k], m, p.data(),
                                     width, s.data(), in.data(), pr.data(), bo.data(), po.data());
            if (one != 0) { if (first_bad < 0) first_bad = k; continue; }
            if (rc != 0) continue;
            for (int j = 0; j < m; j++) {
                const int i = at[j];
                if (s[j] != skip[i] || in[j] != inside[i] || pr[j] != pre[i] || bo[j] != border[i] || po[j] != post[i]) {
                    std::printf("round %d tree %d point %d differs\n", round, k, i);
                    return 1;
                }
                compared++;
            }
        }
        if ((rc != 0) != (first_bad >= 0) || (rc != 0 && found[1] != first_bad)) {
            std::printf("round %d: status %d names tree %d, the per-tree calls name %d\n", round, rc, found[1], first_bad);
            return 1;
        }
        if (rc != 0) {
            refused++;
            for (int i = 0; i < n; i++)
                if (skip[i] != 0x5A || pre[i] != 0x5A5A) { std::printf("round %d: a refusal wrote\n", round); return 1; }
        }
    }
    std::printf("extend_forest_host: %d points equal the per-tree functions, %d forests refused with the right tree\n", compared, refused);
    return compared > 1000 && refused > 10 ? 0 : 1;
}
#endif
