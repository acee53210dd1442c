// Host build of the regularize / settle sweep over a forest (hpmvs_amd/csrc/octree.hpp: process_regularized, process_removed,
// process_split, process_child_key, process_op_count, locate_versioned, regularize_probe / _err2 / _flatness, process_sequential)
// as the kernels of kernel_process_forest.hip apply them.  What the refinement decides (support, which children survive, their
// refined centres) is an input here.  tests/test_cpu_process_forest.py pins it to the sequential loop on the pointer tree.
// Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared process_forest_host.cpp
// Stand-alone (a self-check on forests it draws itself, for a sanitizer run):
//        g++ -std=c++11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -DPROCESS_FOREST_MAIN process_forest_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hpmvs_amd/csrc/octree.hpp"

using namespace hpmvs::octree;

extern "C" {

constexpr int kFoundOffsets = 8, kFoundCell = 100;   // beside kBadKey / kBadTwice / kBadOrphan; a cell's kind k is kFoundCell + k

// roots: [n_trees][4].  ops / op_subtract: room for 5 n.  Returns 0, or -2 with nothing written but found[0] = what and found[1] =
// the offending tree or cell.
int pf_process(int n_trees, const float* roots, const int32_t* branch_first, const int32_t* leaf_first, const uint64_t* branch_key,
               const uint64_t* leaf_key, const float* leaf_patch_center, int n, const float* center, const float* normal, const float* cam_x,
               const uint8_t* ref_ok, const int32_t* cell_tree, const uint64_t* cell_key, float* flatness, const uint8_t* final_level,
               const int32_t* support, const uint8_t* child_ok, const float* child_center, uint8_t* removed, uint8_t* split, uint8_t* children,
               uint64_t* child_key, int32_t* n_neighbours, uint64_t* neighbour_key, int32_t* ops, uint8_t* op_subtract, int32_t* n_ops,
               int32_t* found) {
    found[0] = found[1] = 0;
    if (n_trees == 0) return n == 0 ? (*n_ops = 0, 0) : (found[0] = kFoundCell + (int)kCellTree, found[1] = 0, -2);
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
    // the sweep writes as it goes: it runs on copies, so that a refusal leaves the caller's arrays alone
    std::vector<float> fl(flatness, flatness + n);
    std::vector<uint8_t> rm(n), sp(n), ch(4 * (size_t)n);
    std::vector<uint64_t> ck(4 * (size_t)n), nk(24 * (size_t)n);
    std::vector<int32_t> nn(n), op;
    std::vector<uint8_t> sub;
    const uint32_t v = process_sequential(n_trees, trees.data(), leaf_first, leaf_patch_center, n, center, normal, cam_x, ref_ok, cell_tree,
                                          cell_key, fl.data(), final_level, support, child_ok, child_center, rm.data(), sp.data(), ch.data(),
                                          ck.data(), nn.data(), nk.data(), &op, &sub);
    if (v != kForestGood) { found[0] = kFoundCell + (int)(v & 7u); found[1] = (int32_t)(v >> 3); return -2; }
    if (n) {
        memcpy(flatness, fl.data(), 4 * (size_t)n); memcpy(removed, rm.data(), n); memcpy(split, sp.data(), n);
        memcpy(children, ch.data(), 4 * (size_t)n); memcpy(child_key, ck.data(), 32 * (size_t)n);
        memcpy(n_neighbours, nn.data(), 4 * (size_t)n); memcpy(neighbour_key, nk.data(), 192 * (size_t)n);
    }
    *n_ops = (int32_t)op.size();
    if (!op.empty()) { memcpy(ops, op.data(), 4 * op.size()); memcpy(op_subtract, sub.data(), sub.size()); }
    return 0;
}

}  // extern "C"

#ifdef PROCESS_FOREST_MAIN
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }
static float unit() { return (float)(rnd() % 100001) / 100000.0f - 0.5f; }

// Forests of trees cut evenly to depth 3 (three leaves of four nonempty, two of three of those a cell): the sweep must keep its own
// invariants -- op counts, children only under split cells, child keys below their cell, neighbours distinct -- and a second
// run on the same inputs must give the same bytes.  Then the refusals.
int main() {
    long cells = 0, regs = 0, opsum = 0, refused = 0;
    for (int round = 0; round < 60; round++) {
        const int T = (int)(rnd() % 7);
        std::vector<float> roots, lpc;
        std::vector<int32_t> bf(1, 0), lf(1, 0), ct;
        std::vector<uint64_t> bk, lk, ckey;
        for (int k = 0; k < T; k++) {
            const float root[4] = {unit(), unit(), unit(), 8.0f};
            roots.insert(roots.end(), root, root + 4);
            const Cell rc{{root[0], root[1], root[2]}, root[3]};
            if (k != 1) {
                for (uint64_t a = 0; a < 8; a++) { bk.push_back(8 | a); for (uint64_t b = 0; b < 8; b++) bk.push_back(((8 | a) << 3) | b); }
                for (uint64_t key = 512; key < 1024; key++) {
                    if (rnd() % 4 == 0) continue;
                    const Cell c = key_cell(rc, key);
                    lk.push_back(key);
                    for (int j = 0; j < 3; j++) lpc.push_back(c.c[j] + unit() * c.w * (j == 2 ? 0.2f : 0.9f));
                    if (rnd() % 3) { ct.push_back(k); ckey.push_back(key); }
                }
            }
            bf.push_back((int32_t)bk.size());
            lf.push_back((int32_t)lk.size());
        }
        const int n = (int)ct.size();
        std::vector<float> cen(4 * (size_t)n), nor(4 * (size_t)n), cx(3 * (size_t)n), fl(n), cc(12 * (size_t)n);
        std::vector<uint8_t> ref_ok(n, 1), fin(n), cok(4 * (size_t)n);
        std::vector<int32_t> sup(n);
        for (int i = 0; i < n; i++) {
            const Cell c = key_cell(Cell{{roots[4 * ct[i]], roots[4 * ct[i] + 1], roots[4 * ct[i] + 2]}, 8.0f}, ckey[i]);
            for (int j = 0; j < 3; j++) { cen[4 * i + j] = c.c[j] + unit() * c.w * 0.5f; nor[4 * i + j] = j == 2 ? 1.0f : unit() * 0.2f; cx[3 * i + j] = j == 0 ? 1.0f : 0.0f; }
            const uint32_t r = rnd() % 8;
            fl[i] = r < 3 ? -1.0f : r == 3 ? 2.5f : r == 4 ? 2.6f : r == 5 ? __builtin_nanf("") : (float)(rnd() % 300) / 100.0f;
            fin[i] = rnd() % 2; sup[i] = (int32_t)(rnd() % 4);
            for (int k = 0; k < 4; k++) {
                cok[4 * i + k] = rnd() % 2;
                for (int j = 0; j < 3; j++) cc[3 * (4 * i + k) + j] = (k == 1 && rnd() % 2) ? cc[3 * (4 * i) + j] : c.c[j] + unit() * c.w * 0.99f;
            }
        }
        if (round % 6 == 5 && n > 4) {   // refusals: a bad tree id, a key that is no leaf, a leaf twice, a bad reference image
            const int kind = (round / 6) % 4, at = 1 + (int)(rnd() % (n - 2));
            if (kind == 0) ct[at] = T;
            else if (kind == 1) ckey[at] = 9;
            else if (kind == 2) { ct[at] = ct[at - 1]; ckey[at] = ckey[at - 1]; }
            else { fl[at] = -1.0f; ref_ok[at] = 0; }
            std::vector<float> f2(fl);
            std::vector<uint8_t> rm(n, 0x5A), sp(n, 0x5A), ch(4 * (size_t)n, 0x5A), sub(5 * (size_t)n);
            std::vector<uint64_t> ck(4 * (size_t)n), nk(24 * (size_t)n);
            std::vector<int32_t> nn(n), op(5 * (size_t)n);
            int32_t n_ops = -1, found[2];
            const int rc = pf_process(T, roots.data(), bf.data(), lf.data(), bk.data(), lk.data(), lpc.data(), n, cen.data(), nor.data(), cx.data(),
                                      ref_ok.data(), ct.data(), ckey.data(), f2.data(), fin.data(), sup.data(), cok.data(), cc.data(), rm.data(),
                                      sp.data(), ch.data(), ck.data(), nn.data(), nk.data(), op.data(), sub.data(), &n_ops, found);
            if (rc != -2 || found[1] != at || found[0] != kFoundCell + (kind == 3 ? 4 : kind) || rm[0] != 0x5A || n_ops != -1 ||
                memcmp(f2.data(), fl.data(), 4 * (size_t)n)) {
                std::printf("round %d: refusal kind %d at %d came back as %d (%d, %d)\n", round, kind, at, rc, found[0], found[1]);
                return 1;
            }
            refused++;
            continue;
        }
        std::vector<float> f1(fl), f2(fl);
        std::vector<uint8_t> rm(n), sp(n), ch(4 * (size_t)n), sub(5 * (size_t)n), rm2(n), sp2(n), ch2(4 * (size_t)n), sub2(5 * (size_t)n);
        std::vector<uint64_t> ck(4 * (size_t)n), nk(24 * (size_t)n), ck2(4 * (size_t)n), nk2(24 * (size_t)n);
        std::vector<int32_t> nn(n), op(5 * (size_t)n), nn2(n), op2(5 * (size_t)n);
        int32_t n_ops = 0, n_ops2 = 0, found[2];
        int rc = pf_process(T, roots.data(), bf.data(), lf.data(), bk.data(), lk.data(), lpc.data(), n, cen.data(), nor.data(), cx.data(),
                            ref_ok.data(), ct.data(), ckey.data(), f1.data(), fin.data(), sup.data(), cok.data(), cc.data(), rm.data(), sp.data(),
                            ch.data(), ck.data(), nn.data(), nk.data(), op.data(), sub.data(), &n_ops, found);
        rc |= pf_process(T, roots.data(), bf.data(), lf.data(), bk.data(), lk.data(), lpc.data(), n, cen.data(), nor.data(), cx.data(),
                         ref_ok.data(), ct.data(), ckey.data(), f2.data(), fin.data(), sup.data(), cok.data(), cc.data(), rm2.data(), sp2.data(),
                         ch2.data(), ck2.data(), nn2.data(), nk2.data(), op2.data(), sub2.data(), &n_ops2, found);
        if (rc != 0 || n_ops != n_ops2 || (n && (memcmp(f1.data(), f2.data(), 4 * (size_t)n) || memcmp(nk.data(), nk2.data(), 192 * (size_t)n)))) {
            std::printf("round %d: status %d, or two runs differ\n", round, rc);
            return 1;
        }
        int want_ops = 0;
        for (int i = 0; i < n; i++) {
            int nc = 0;
            for (int k = 0; k < 4; k++) {
                if (!ch[4 * i + k]) { if (ck[4 * i + k]) { std::printf("round %d cell %d: a key without a child\n", round, i); return 1; } continue; }
                nc++;
                if (!sp[i] || (ck[4 * i + k] >> 3) != ckey[i]) { std::printf("round %d cell %d: a child outside its split cell\n", round, i); return 1; }
            }
            const bool reg = fl[i] < 0.0f;
            if (reg != (nn[i] != -2) || (reg && (rm[i] || sp[i])) || (rm[i] && sp[i])) { std::printf("round %d cell %d: decisions clash\n", round, i); return 1; }
            for (int a = 0; a < (reg ? nn[i] : 0); a++)
                for (int b = 0; b < a; b++)
                    if (nk[24 * i + a] == nk[24 * i + b] || !nk[24 * i + a]) { std::printf("round %d cell %d: neighbours repeat\n", round, i); return 1; }
            want_ops += process_op_count(rm[i] != 0, sp[i] != 0, nc);
            regs += reg;
        }
        if (want_ops != n_ops) { std::printf("round %d: %d ops, the decisions make %d\n", round, n_ops, want_ops); return 1; }
        cells += n;
        opsum += n_ops;
    }
    std::printf("process_forest_host: %ld cells (%ld regularized), %ld setDepths calls, %ld refusals named the right cell\n", cells, regs, opsum, refused);
    return cells > 1000 && regs > 300 && opsum > 300 && refused >= 8 ? 0 : 1;
}
#endif
