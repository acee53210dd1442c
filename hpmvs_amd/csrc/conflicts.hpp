// conflicts.hpp -- the conflict graph of one extend level (include/hpmvs_amd.h: hpmvs_level_conflicts_batch,
// hpmvs_conflicts_from_footprints): which node's setDepths would write a depth-map cell that another node's gates
// read.  ONE statement of the cells a footprint names, used by the kernels (kernel_conflicts.hip) and by the host restatement
// conflicts_sequential below, as octree.hpp does for border_forest_sequential.  No HIP types: the header compiles with g++.
//
// Footprints are the arrays of hpmvs_depth_footprints_batch (n nodes, rows of M ids, V views):
//   wr [n][M][4]  view, level, x, y of the cell setDepths would write            (view < 0: none)
//   fr [n][M][4]  view, level, x, y of the cell pixelFreeTests reads             (view < 0: none)
//   at [n][M][3]  view, ix0, iy0: depthTests' 3x3 level-0 pixel block            (view < 0: none)
//   vb [n][V][3]  examined?, ix0, iy0: viewBlockTest's block in view v
// Only the first n_images[i] (clamped to 0 .. M) entries of a row of wr / fr / at count.  A block from (ix0, iy0) covers, on every
// level l < n_levels, the cells x0 >> (1 + l) .. x1 >> (1 + l) with x1 = ix0 + 2, x0 = max(ix0, 0) (likewise y); no block when
// x1 < 0 or y1 < 0.  Ignored: an entry with view < 0 or view >= V, a wr / fr entry with a level outside [0, n_levels), and a cell
// or block outside [0, 2^24) -- no map has such a cell, and the key has 24 bits per coordinate.
//
// Nodes are candidates or events (is_event[i] != 0; a null is_event: all candidates).  An event has writes and NO reads.
//   flow[i], i a candidate: nodes j < i of either kind that write a cell i reads
//   flow[i], i an event:    candidates j < i that write a cell i writes
//   anti[i], i a candidate: candidates j < i that read a cell i writes, and events j < i that write a cell i writes
//   anti[i], i an event:    candidates j < i that read a cell i writes
// No edge between two events, no node its own neighbour.  Both lists in CSR, every list ascending without duplicates.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CONFLICTS_HD __host__ __device__
#else
#define CONFLICTS_HD
#endif

namespace conflicts {

constexpr int kMaxViews = 8191;                      // (view << 3 | level) takes the key's top 16 bits; all ones is never a key
constexpr int kCoordLimit = 1 << 24;                 // cells per side the key can name
constexpr unsigned long long kMaxRawPairs = 1ull << 30;   // more matches (item_matches; they bound the raw pairs): HPMVS_ERR_STATE
constexpr unsigned long long kAntiBit = 1ull << 63;  // a pair is list << 63 | owner << 32 | member, the owner being the LATER node

struct Footprints {
    int n, M, V, n_levels;
    const int32_t* n_images;
    const int32_t *wr, *fr, *at, *vb;
    const uint8_t* is_event;   // nullable
};

// A depth-map cell as a key: (view, pyramid level, x, y) -- hpmvs_host.cpp's cell_key.  For one (view, level, x) the cells of a
// column ys .. ye are CONSECUTIVE keys, which is what lets a block's rectangle be at most two key ranges.
CONFLICTS_HD inline unsigned long long cell_key(int view, int level, int x, int y) {
    return ((unsigned long long)(((unsigned)view << 3) | (unsigned)level) << 48) | ((unsigned long long)((unsigned)x & 0xFFFFFFu) << 24) |
           (unsigned long long)((unsigned)y & 0xFFFFFFu);
}
CONFLICTS_HD inline int images_of(const Footprints& F, int i) {
    const int m = F.n_images[i];
    return m < 0 ? 0 : (m > F.M ? F.M : m);
}
CONFLICTS_HD inline bool is_event(const Footprints& F, int i) { return F.is_event && F.is_event[i]; }
// a wr / fr entry (view, level, x, y) that names a cell
CONFLICTS_HD inline bool cell_entry(const Footprints& F, const int32_t* e, unsigned long long& key) {
    if (e[0] < 0 || e[0] >= F.V || e[1] < 0 || e[1] >= F.n_levels) return false;
    if (e[2] < 0 || e[2] >= kCoordLimit || e[3] < 0 || e[3] >= kCoordLimit) return false;
    key = cell_key(e[0], e[1], e[2], e[3]);
    return true;
}
// the cell node i would write for its attached image k
CONFLICTS_HD inline bool write_key(const Footprints& F, int i, int k, unsigned long long& key) {
    return k < images_of(F, i) && cell_entry(F, F.wr + ((size_t)i * F.M + k) * 4, key);
}

// Inclusive key ranges, at most two (the one or two columns of a block's rectangle on one level).
struct Ranges {
    int n;
    unsigned long long lo[2], hi[2];
};
CONFLICTS_HD inline void block_ranges(const Footprints& F, int view, int ix0, int iy0, int l, Ranges& R) {
    R.n = 0;
    if (view < 0 || view >= F.V) return;
    if (ix0 < -2 || iy0 < -2 || ix0 >= kCoordLimit || iy0 >= kCoordLimit) return;   // (x1 < 0 or y1 < 0: getFullDepth looks nothing up)
    const int x1 = ix0 + 2, y1 = iy0 + 2, x0 = ix0 < 0 ? 0 : ix0, y0 = iy0 < 0 ? 0 : iy0;
    const int xs = x0 >> (1 + l), xe = x1 >> (1 + l), ys = y0 >> (1 + l), ye = y1 >> (1 + l);
    for (int x = xs; x <= xe; x++) { R.lo[R.n] = cell_key(view, l, x, ys); R.hi[R.n] = cell_key(view, l, x, ye); R.n++; }
}
// The items of a node, what one lane looks up at a time.  A candidate's are its READS: item q < M is pixelFreeTests' cell of image
// q; item M + b * n_levels + l is level l of block b, b < M depthTests' block of image b, else viewBlockTest's of view b - M.  An
// event's are its WRITES, one per image.  What an item's cells are looked up among: every other node's writes for a candidate, the
// candidates' writes for an event (conflicts_sequential and the kernels apply that filter to the writer).
CONFLICTS_HD inline int item_count(const Footprints& F, int i) { return is_event(F, i) ? F.M : F.M + (F.M + F.V) * F.n_levels; }
CONFLICTS_HD inline void item_ranges(const Footprints& F, int i, int q, Ranges& R) {
    R.n = 0;
    if (q < F.M) {
        unsigned long long key;
        const bool ok = is_event(F, i) ? write_key(F, i, q, key) : (q < images_of(F, i) && cell_entry(F, F.fr + ((size_t)i * F.M + q) * 4, key));
        if (ok) { R.n = 1; R.lo[0] = R.hi[0] = key; }
        return;
    }
    const int b = (q - F.M) / F.n_levels, l = (q - F.M) - b * F.n_levels;
    if (b < F.M) {
        if (b >= images_of(F, i)) return;
        const int32_t* a = F.at + ((size_t)i * F.M + b) * 3;
        block_ranges(F, a[0], a[1], a[2], l, R);
    } else {
        const int32_t* v = F.vb + ((size_t)i * F.V + (b - F.M)) * 3;
        if (v[0]) block_ranges(F, b - F.M, v[1], v[2], l, R);
    }
}
// The pair a match gives: node i's item met a write of node j.  False: no edge (the node itself, two events, an event's write
// against an event's).  The owner is the later node; flow when the later node is the one whose ITEM it was.
CONFLICTS_HD inline bool pair_of(const Footprints& F, int i, int j, unsigned long long& pair) {
    if (i == j || (is_event(F, i) && is_event(F, j))) return false;
    if (j < i) pair = ((unsigned long long)(unsigned)i << 32) | (unsigned)j;                // flow[i] gets j
    else pair = kAntiBit | ((unsigned long long)(unsigned)j << 32) | (unsigned)i;           // anti[j] gets i
    return true;
}
// first position in the sorted keys [0, count) that is not below `key`
CONFLICTS_HD inline size_t lower_bound_key(const unsigned long long* keys, size_t count, unsigned long long key) {
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first position in the sorted keys [0, count) that is above `key`
CONFLICTS_HD inline size_t upper_bound_key(const unsigned long long* keys, size_t count, unsigned long long key) {
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The write records inside the key ranges of node i's item q, by two bounds per range and no walk.  Every raw pair of the item is
// one of them (the others: the node's own writes, an event's writes met by an event), so the sum over all items -- the level's
// MATCHES -- is what kMaxRawPairs is held against: a hostile input is refused at O(log) per range, before any walk over it.
CONFLICTS_HD inline unsigned long long item_matches(const Footprints& F, int i, int q, const unsigned long long* keys, size_t count) {
    Ranges R;
    item_ranges(F, i, q, R);
    unsigned long long c = 0;
    for (int r = 0; r < R.n; r++) c += upper_bound_key(keys, count, R.hi[r]) - lower_bound_key(keys, count, R.lo[r]);
    return c;
}

// The host restatement: the same records, items and pairs, one node after the other.  Returns false when the matches exceed
// kMaxRawPairs (nothing is written then).
inline bool conflicts_sequential(const Footprints& F, std::vector<uint32_t>& flow_off, std::vector<uint32_t>& flow_adj,
                                 std::vector<uint32_t>& anti_off, std::vector<uint32_t>& anti_adj) {
    const size_t n = (size_t)F.n;
    std::vector<std::pair<unsigned long long, uint32_t> > rec;   // (cell key, writer)
    for (int i = 0; i < F.n; i++)
        for (int k = 0; k < F.M; k++) {
            unsigned long long key;
            if (write_key(F, i, k, key)) rec.emplace_back(key, (uint32_t)i);
        }
    std::sort(rec.begin(), rec.end());
    std::vector<unsigned long long> keys(rec.size());
    for (size_t r = 0; r < rec.size(); r++) keys[r] = rec[r].first;
    auto each_pair = [&](auto&& fn) {
        for (int i = 0; i < F.n; i++) {
            const int items = item_count(F, i);
            for (int q = 0; q < items; q++) {
                Ranges R;
                item_ranges(F, i, q, R);
                for (int c = 0; c < R.n; c++)
                    for (size_t r = lower_bound_key(keys.data(), keys.size(), R.lo[c]); r < keys.size() && keys[r] <= R.hi[c]; r++) {
                        unsigned long long p;
                        if (pair_of(F, i, (int)rec[r].second, p)) fn(p);
                    }
            }
        }
    };
    unsigned long long matches = 0;   // bounded first, as the device does: a hostile input is refused before anything is walked
    for (int i = 0; i < F.n; i++)
        for (int q = 0, items = item_count(F, i); q < items; q++) matches += item_matches(F, i, q, keys.data(), keys.size());
    if (matches > kMaxRawPairs) return false;
    std::vector<unsigned long long> pairs;
    pairs.reserve((size_t)matches);
    each_pair([&](unsigned long long p) { pairs.push_back(p); });
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    flow_off.assign(n + 1, 0); anti_off.assign(n + 1, 0);
    flow_adj.clear(); anti_adj.clear();
    for (unsigned long long p : pairs) {
        const size_t owner = (size_t)((p & ~kAntiBit) >> 32);
        if (p & kAntiBit) { anti_off[owner + 1]++; anti_adj.push_back((uint32_t)p); }
        else { flow_off[owner + 1]++; flow_adj.push_back((uint32_t)p); }
    }
    for (size_t i = 0; i < n; i++) { flow_off[i + 1] += flow_off[i]; anti_off[i + 1] += anti_off[i]; }
    return true;
}

}  // namespace conflicts
