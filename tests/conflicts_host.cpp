// The g++ build of hpmvs_amd/csrc/conflicts.hpp's conflicts_sequential behind a C entry (tests/conflicts_ref.py loads it): the
// host restatement of hpmvs_conflicts_from_footprints, same arguments, same capacity contract.  Returns 0, -2 when a capacity does
// not suffice (offsets and totals written), -3 when the matches, which bound the raw pairs, exceed the limit (nothing written).
#include "../hpmvs_amd/csrc/conflicts.hpp"

#include <cstring>

extern "C" int cf_conflicts(int n, int M, int V, int n_levels, const int32_t* n_images, const int32_t* wr, const int32_t* fr, const int32_t* at,
                            const int32_t* vb, const uint8_t* is_event, uint32_t* flow_off, uint32_t* flow_adj, size_t cap_flow,
                            uint32_t* anti_off, uint32_t* anti_adj, size_t cap_anti, uint32_t* n_flow, uint32_t* n_anti) {
    conflicts::Footprints F;
    F.n = n; F.M = M; F.V = V; F.n_levels = n_levels;
    F.n_images = n_images; F.wr = wr; F.fr = fr; F.at = at; F.vb = vb; F.is_event = is_event;
    std::vector<uint32_t> fo, fa, ao, aa;
    if (!conflicts::conflicts_sequential(F, fo, fa, ao, aa)) return -3;
    std::memcpy(flow_off, fo.data(), 4 * fo.size());
    std::memcpy(anti_off, ao.data(), 4 * ao.size());
    *n_flow = (uint32_t)fa.size(); *n_anti = (uint32_t)aa.size();
    if (fa.size() > cap_flow || aa.size() > cap_anti) return -2;
    if (!fa.empty()) std::memcpy(flow_adj, fa.data(), 4 * fa.size());
    if (!aa.empty()) std::memcpy(anti_adj, aa.data(), 4 * aa.size());
    return 0;
}
