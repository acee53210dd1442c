// The g++ build of hpmvs_amd/csrc/level_walk.hpp's walk_by_rounds behind a C entry (tests/test_cpu_level_walk.py loads it): the
// host restatement of hpmvs_level_walk_batch with the device behind two callbacks, as frontier._walk has it.  The conflict graph is
// the caller's, over the nodes (the events and the refined candidates in queue order).  rounds [n]: rounds per wave.  Returns 0, or
// -1 for a flag byte that cannot occur (nothing written), -2 when a round decided nothing or the waves exceeded n.
#include "../hpmvs_amd/csrc/level_walk.hpp"

extern "C" int lw_walk(int n, int min_images, const uint8_t* flags, const int32_t* set, const unsigned long long* pre,
                       const unsigned long long* post, const uint32_t* flow_off, const uint32_t* flow_adj, const uint32_t* anti_off,
                       const uint32_t* anti_adj, const int32_t* n_images, int32_t* stage, int32_t* counts, uint8_t* accepted, int32_t* wave,
                       int32_t* n_waves, int32_t* rounds, void (*gates)(int, const int32_t*, int32_t*),
                       void (*apply)(int, const int32_t*, int)) {
    for (int i = 0; i < n; i++)
        if (!level_walk::flags_valid(flags[i])) return -1;
    level_walk::Level L;
    L.n = n; L.min_images = min_images; L.flags = flags; L.set = set; L.pre = pre; L.post = post;
    L.flow_off = flow_off; L.flow_adj = flow_adj; L.anti_off = anti_off; L.anti_adj = anti_adj;
    level_walk::HostLevel H;
    H.build(L);
    std::vector<int> r;
    const bool ok = level_walk::walk_by_rounds(
        L, n_images, stage, counts, accepted, wave, n_waves, &r,
        [&](const std::vector<int>& items, std::vector<int32_t>& vbf) { gates((int)items.size(), items.data(), vbf.data()); },
        [&](const std::vector<int>& ops, bool any_event) { apply((int)ops.size(), ops.data(), any_event ? 1 : 0); });
    for (size_t w = 0; w < r.size() && w < (size_t)n; w++) rounds[w] = r[w];
    return ok ? 0 : -2;
}
