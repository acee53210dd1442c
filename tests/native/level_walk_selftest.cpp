// Stand-alone check of hpmvs_amd/csrc/level_walk.hpp's walk_by_rounds, built with -fsanitize=address,undefined and run as a program
// (tests/test_cpu_level_walk.py): random queues of candidates and subtraction events over a toy of integer "maps" -- an accepted
// candidate increments its write cells, an event resets its cells, a candidate's counts are a function of its read cells -- against
// the obvious sequential loop over the same queue: one item after the other, every count read from the maps as they are.  Key sets,
// border candidates, candidates without a pre key, leaves taken at the start.  Prints "<k> failures"; exit status 0 only for k == 0.
#include "../../hpmvs_amd/csrc/level_walk.hpp"

#include <cstdio>
#include <map>
#include <set>

namespace {
namespace lw = level_walk;

unsigned long long state = 0x9E3779B97F4A7C15ull;
int rnd(int m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int)((state >> 33) % (unsigned long long)m); }

const int MIN = 3;

bool meets(const std::set<int>& a, const std::set<int>& b) {
    for (int c : a) if (b.count(c)) return true;
    return false;
}

int run(int n, int n_cells, int n_keys, int n_sets, int event_every) {
    std::vector<uint8_t> flags((size_t)n);
    std::vector<int32_t> set((size_t)n), thr((size_t)n), n_images((size_t)n, 4), stage((size_t)n, 1);
    std::vector<unsigned long long> pre((size_t)n), post((size_t)n);
    std::vector<std::set<int> > R((size_t)n), W((size_t)n);
    std::set<std::pair<int, unsigned long long> > occ0;
    for (int k = 0; k < 5; k++) occ0.insert({rnd(n_sets), (unsigned long long)rnd(n_keys)});
    for (int i = 0; i < n; i++) {
        set[i] = rnd(n_sets); pre[i] = (unsigned long long)rnd(n_keys); post[i] = (unsigned long long)rnd(n_keys); thr[i] = 1 + rnd(4);
        for (int k = 1 + rnd(3); k > 0; k--) W[i].insert(rnd(n_cells));
        if (event_every && i % event_every == event_every - 1) { flags[i] = lw::kEvent; stage[i] = 0; continue; }
        for (int k = 1 + rnd(5); k > 0; k--) R[i].insert(rnd(n_cells));
        uint8_t f = 0;
        if (rnd(100) < 85) f |= lw::kRefined;
        if ((f & lw::kRefined) && rnd(100) < 12) f |= lw::kBorder;
        if (rnd(100) < 90) { f |= lw::kHasPre; if (occ0.count({set[i], pre[i]})) f |= lw::kPreTaken; }
        if (lw::has_post_record(f) && occ0.count({set[i], post[i]})) f |= lw::kPostTaken;
        flags[i] = f;
    }
    std::vector<int> maps0((size_t)n_cells);
    for (int c = 0; c < n_cells; c++) maps0[c] = rnd(2);
    auto count = [&](const std::vector<int>& maps, int i, int32_t* vbf) {
        int s = 0;
        for (int c : R[i]) s += maps[c];
        vbf[0] = s < thr[i] ? MIN : 0; vbf[1] = (s == 0 && R[i].size() > 3) ? MIN : 0; vbf[2] = s != 1 ? 4 : 2;
    };
    auto enter = [&](std::vector<int>& maps, int i) {
        for (int c : W[i]) maps[c] = lw::is_event(flags[i]) ? 0 : maps[c] + 1;
    };
    // the sequential loop
    std::vector<int> maps = maps0;
    std::vector<int32_t> want = stage;
    std::vector<uint8_t> want_acc((size_t)n, 0);
    auto occ = occ0;
    for (int i = 0; i < n; i++) {
        const uint8_t f = flags[i];
        if (lw::is_event(f)) { enter(maps, i); continue; }
        if ((f & lw::kHasPre) && occ.count({set[i], pre[i]})) { want[i] = 20; continue; }
        if (!(f & lw::kRefined)) continue;
        int32_t c[3];
        count(maps, i, c);
        if (!(c[0] >= MIN)) want[i] = 23;
        else if (!(c[1] < MIN)) want[i] = 24;
        else if (!(c[2] >= MIN - 1 && c[2] * 1.0 / 4 > 0.75)) want[i] = 25;
        else if (f & lw::kBorder) want[i] = 27;
        else if (occ.count({set[i], post[i]})) want[i] = 26;
        else { occ.insert({set[i], post[i]}); want[i] = 0; want_acc[i] = 1; enter(maps, i); }
    }
    // the graph over the nodes, by the definition of conflicts.hpp
    std::vector<int> nodes;
    for (int i = 0; i < n; i++) if (lw::is_node(flags[i])) nodes.push_back(i);
    std::vector<uint32_t> fo(1, 0), fa, ao(1, 0), aa;
    for (size_t a = 0; a < nodes.size(); a++) {
        const int i = nodes[a];
        const bool ei = lw::is_event(flags[i]);
        for (size_t b = 0; b < a; b++) {
            const int j = nodes[b];
            const bool ej = lw::is_event(flags[j]);
            if (ei) {
                if (!ej && meets(W[j], W[i])) fa.push_back((uint32_t)b);
                if (!ej && meets(R[j], W[i])) aa.push_back((uint32_t)b);
            } else {
                if (meets(W[j], R[i])) fa.push_back((uint32_t)b);
                if (ej ? meets(W[j], W[i]) : meets(R[j], W[i])) aa.push_back((uint32_t)b);
            }
        }
        fo.push_back((uint32_t)fa.size()); ao.push_back((uint32_t)aa.size());
    }
    fa.push_back(0); aa.push_back(0);   // (never empty arrays)
    lw::Level L;
    L.n = n; L.min_images = MIN; L.flags = flags.data(); L.set = n_sets > 1 ? set.data() : nullptr; L.pre = pre.data(); L.post = post.data();
    L.flow_off = fo.data(); L.flow_adj = fa.data(); L.anti_off = ao.data(); L.anti_adj = aa.data();
    lw::HostLevel H;
    H.build(L);
    std::vector<int> maps2 = maps0, rounds;
    std::vector<int32_t> got = stage, counts(3 * (size_t)n), wave((size_t)n);
    std::vector<uint8_t> acc((size_t)n);
    int32_t n_waves = -1;
    const bool ok = lw::walk_by_rounds(
        L, n_images.data(), got.data(), counts.data(), acc.data(), wave.data(), &n_waves, &rounds,
        [&](const std::vector<int>& items, std::vector<int32_t>& vbf) { for (size_t k = 0; k < items.size(); k++) count(maps2, items[k], &vbf[3 * k]); },
        [&](const std::vector<int>& ops, bool) { for (int i : ops) enter(maps2, i); });
    int bad = ok ? 0 : 1, most = 0;
    for (int i = 0; i < n; i++) bad += got[i] != want[i] || acc[i] != want_acc[i] || (n_waves > 0 && (wave[i] < 1 || wave[i] > n_waves));
    bad += maps2 != maps;
    for (int r : rounds) most = std::max(most, r);
    std::printf("n %d cells %d keys %d sets %d events 1/%d: %d waves, at most %d rounds in a wave, %d differences\n", n, n_cells, n_keys, n_sets,
                event_every, (int)n_waves, most, bad);
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    bad += run(0, 1, 1, 1, 0);
    bad += run(1, 1, 1, 1, 0);
    bad += run(2, 1, 1, 1, 2);
    for (int k = 0; k < 40; k++) {
        bad += run(60 + rnd(60), 40, 10, 1 + rnd(4), 0);
        bad += run(60 + rnd(60), 12 + rnd(200), 6 + rnd(6), 1 + rnd(4), 3 + rnd(3));
    }
    bad += run(80, 12, 4, 1, 4);
    bad += run(700, 300, 40, 3, 5);
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
