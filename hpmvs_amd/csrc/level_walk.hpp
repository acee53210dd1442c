// level_walk.hpp -- the wave walk of one extend level as a rule over EARLIER NEIGHBOURS (include/hpmvs_amd.h:
// hpmvs_level_walk_batch).  ONE statement of what an item of a wave becomes, used by the kernels
// (kernel_level_walk.hip) and by the host restatement walk_by_rounds below, as conflicts.hpp is shared.  No HIP types: the header
// compiles with g++.  hpmvs_amd/frontier.py's _walk states the same walk over six sets; this header states it without them.
//
// The level's queue holds n ITEMS in the reference's order: subtraction events (kEvent) and candidates.  A candidate has
//   kRefined    it was refined (it reads and writes map cells; its row of the batch counts)
//   kBorder     refined and outside its tree's root: past the three counts it gets stage 27, writes no depth, occupies no leaf
//   kHasPre     it has a leaf key before refinement (C++ preIn); kPreTaken: that leaf is taken when the level starts
//   kPostTaken  the leaf of the refined patch is taken when the level starts
// and set[i] (the tree its keys belong to: keys are equal only within one set), pre[i], post[i].  The level's conflict graph
// (conflicts.hpp) is over the NODES -- the events and the refined candidates, in queue order: node_of / item_of.
//
// A wave decides its pending items; an item's outcome is a function of this wave's gate counts and of the outcomes of EARLIER
// pending items it shares a map cell (flow / anti) or a leaf key with, so an item decides once none of those that can still change
// its outcome is undecided, and a wave is evaluated in ROUNDS.  "Writes" of a candidate count only if it is refined and not border, "reads" only if it is refined.
//   event e      kDeferEvent if a candidate of flow[e] is kAccept / kDefer or a candidate of anti[e] is kDefer, else kApply
//   candidate t  1 occ(pre): kPreTaken, or an earlier kAccept of its set with post == pre               -> stage 20
//                2 maybe(pre): an earlier kDefer, refined and not border, of its set with post == pre   -> kDefer
//                3 not refined: final, its preset stage stays
//                4 a node of flow[t] is an event of this wave, or a candidate kAccept / kDefer          -> kDefer
//                5 the counts of this wave's gate pass are written; stage 23 / 24 / 25 by the thresholds, 27 if border
//                6 occ(post)                                                                            -> stage 26
//                7 maybe(post), an earlier kDefer of its set with pre == post, or a node of anti[t] that is a kDefer candidate
//                  or a kDeferEvent                                                                     -> kDefer, counts back to -1
//                8 kAccept, stage 0
// Between waves (next_wave_state) a deferred item becomes undecided again, an accepted candidate stays an occupant of its leaf
// (kAcceptOld) and everything else is done: its writes are in the maps the next wave's counts are read from.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEVEL_WALK_HD __host__ __device__
#else
#define LEVEL_WALK_HD
#endif

namespace level_walk {

constexpr uint8_t kEvent = 1, kRefined = 2, kBorder = 4, kHasPre = 8, kPreTaken = 16, kPostTaken = 32, kFlagMask = 63;   // HPMVS_WALK_*

// an item's state in the walk; kUndecided .. kDeferEvent are a wave's outcomes, the last two what they leave for later waves
enum : uint8_t { kUndecided = 0, kReject = 1, kAccept = 2, kDefer = 3, kApply = 4, kDeferEvent = 5, kAcceptOld = 6, kDone = 7 };

constexpr uint32_t kNoSet = 0xFFFFFFFFu;   // the set of a key record that is none (sorted behind every set)

// a flag byte that can occur: no unknown bit, an event neither refined nor border
LEVEL_WALK_HD inline bool flags_valid(uint8_t f) { return !(f & ~kFlagMask) && !((f & kEvent) && (f & (kRefined | kBorder))); }
LEVEL_WALK_HD inline bool is_event(uint8_t f) { return (f & kEvent) != 0; }
LEVEL_WALK_HD inline bool is_node(uint8_t f) { return (f & (kEvent | kRefined)) != 0; }
// the key records of a candidate: its pre key guards, its post key occupies
LEVEL_WALK_HD inline bool has_pre_record(uint8_t f) { return !(f & kEvent) && (f & kHasPre); }
LEVEL_WALK_HD inline bool has_post_record(uint8_t f) { return !(f & kEvent) && (f & kRefined) && !(f & kBorder); }

LEVEL_WALK_HD inline uint8_t next_wave_state(uint8_t s) {
    return (s == kDefer || s == kDeferEvent) ? kUndecided : s == kAccept ? kAcceptOld : (s == kReject || s == kApply) ? kDone : s;
}

// One level as the rule reads it.  The key records are the candidates' (set, key, item << 1 | role) -- role 0: a pre key, 1: a post
// key -- sorted; first_pre[t] / first_post[t]: the first record of (set[t], pre[t]) / (set[t], post[t]).
struct Level {
    int n, min_images;
    const uint8_t* flags;
    const int32_t* set;                       // nullable: one set
    const unsigned long long *pre, *post;
    const int32_t *node_of, *item_of;         // item -> node (-1: none), node -> item
    const uint32_t *flow_off, *flow_adj, *anti_off, *anti_adj;   // over nodes (only read for items with a node)
    uint32_t n_rec;
    const uint32_t* rec_set;
    const unsigned long long* rec_key;
    const uint32_t* rec_val;
    const uint32_t *first_pre, *first_post;
};

LEVEL_WALK_HD inline uint32_t set_of(const Level& L, int i) { return L.set ? (uint32_t)L.set[i] : 0u; }
// first record not below (set, key)
LEVEL_WALK_HD inline uint32_t first_record(const uint32_t* rec_set, const unsigned long long* rec_key, uint32_t n_rec, uint32_t set,
                                           unsigned long long key) {
    uint32_t lo = 0, hi = n_rec;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rec_set[mid] < set || (rec_set[mid] == set && rec_key[mid] < key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Outcome {
    uint8_t state;
    int32_t stage;    // < 0: the stage stays
    bool counts;      // the gate counts are the candidate's counts (else they are -1)
};

// what the earlier items of one key say: the records of (set, key) from `first`, of items before t
struct KeyFacts { bool wait, occupied, maybe, guarded; };
LEVEL_WALK_HD inline KeyFacts key_facts(const Level& L, const uint8_t* st, uint32_t first, uint32_t set, unsigned long long key, int t,
                                        bool pre_roles) {
    KeyFacts k = {false, false, false, false};
    for (uint32_t r = first; r < L.n_rec && L.rec_set[r] == set && L.rec_key[r] == key; r++) {
        const int j = (int)(L.rec_val[r] >> 1);
        if (j >= t) break;   // (ascending by item within a key)
        const bool post = (L.rec_val[r] & 1u) != 0;
        if (!post && !pre_roles) continue;
        const uint8_t s = st[j];
        if (s == kUndecided) k.wait = true;
        if (post) { k.occupied |= s == kAccept || s == kAcceptOld; k.maybe |= s == kDefer; }
        else k.guarded |= s == kDefer;
    }
    return k;
}

// THE RULE.  False: the outcome of item i still hangs on an earlier neighbour that is undecided (`o` is not written).  st: the items'
// states; v, b, f: this wave's counts of a refined candidate (not read otherwise); n_images: its image count.
// An undecided neighbour is waited for only where it can still change the outcome: the facts are monotone -- an occupant, a hit
// stay -- and the tests have an order, so a test that already holds decides whatever the undecided neighbours of LATER tests, and
// of this one, become.  An undecided event in a candidate's flow list is a hit as it stands: applied or deferred, it counts.
LEVEL_WALK_HD inline bool decide(const Level& L, const uint8_t* st, int i, int v, int b, int f, int n_images, Outcome& o) {
    const uint8_t fl = L.flags[i];
    bool flow_wait = false, anti_wait = false, flow_hit = false, anti_hit = false;
    const int node = L.node_of[i];
    if (node >= 0) {
        for (uint32_t q = L.flow_off[node]; q < L.flow_off[node + 1]; q++) {
            const int m = L.item_of[L.flow_adj[q]];
            const uint8_t s = st[m], fm = L.flags[m];
            if (is_event(fm)) flow_hit |= s == kUndecided || s == kApply || s == kDeferEvent;   // (an event's flow list holds no event)
            else if (!(fm & kBorder)) { flow_wait |= s == kUndecided; flow_hit |= s == kAccept || s == kDefer; }
        }
        for (uint32_t q = L.anti_off[node]; q < L.anti_off[node + 1]; q++) {
            const int m = L.item_of[L.anti_adj[q]];
            const uint8_t s = st[m];
            anti_wait |= s == kUndecided;
            anti_hit |= is_event(L.flags[m]) ? s == kDeferEvent : s == kDefer;
        }
    }
    o.stage = -1; o.counts = false;
    if (is_event(fl)) {
        if (flow_hit || anti_hit) { o.state = kDeferEvent; return true; }
        if (flow_wait || anti_wait) return false;
        o.state = kApply;
        return true;
    }
    const uint32_t set = set_of(L, i);
    if (fl & kHasPre) {
        const KeyFacts pre = key_facts(L, st, L.first_pre[i], set, L.pre[i], i, false);
        if ((fl & kPreTaken) || pre.occupied) { o.state = kReject; o.stage = 20; return true; }
        if (pre.wait) return false;
        if (pre.maybe) { o.state = kDefer; return true; }
    }
    if (!(fl & kRefined)) { o.state = kReject; return true; }
    if (flow_hit) { o.state = kDefer; return true; }
    if (flow_wait) return false;
    o.counts = true; o.state = kReject;
    const int MIN = L.min_images;
    if (!(v >= MIN)) { o.stage = 23; return true; }
    if (!(b < MIN)) { o.stage = 24; return true; }
    if (!(f >= MIN - 1 && f * 1.0 / n_images > 0.75)) { o.stage = 25; return true; }
    if (fl & kBorder) { o.stage = 27; return true; }
    const KeyFacts post = key_facts(L, st, L.first_post[i], set, L.post[i], i, true);
    if ((fl & kPostTaken) || post.occupied) { o.stage = 26; return true; }
    if (post.wait) return false;
    o.stage = -1; o.counts = false;
    if (post.maybe || post.guarded || anti_hit) { o.state = kDefer; return true; }
    if (anti_wait) return false;
    o.counts = true; o.state = kAccept; o.stage = 0;
    return true;
}

// ---- the host restatement ---------------------------------------------------------------------------------------------------------

// The arrays of a Level the caller does not have: the node maps and the sorted key records (the device builds the same with a scan
// and two stable radix sorts).
struct HostLevel {
    std::vector<int32_t> node_of, item_of;
    std::vector<uint32_t> rec_set, rec_val, first_pre, first_post;
    std::vector<unsigned long long> rec_key;
    void build(Level& L) {
        const int n = L.n;
        node_of.assign((size_t)n, -1); item_of.clear();
        for (int i = 0; i < n; i++)
            if (is_node(L.flags[i])) { node_of[(size_t)i] = (int32_t)item_of.size(); item_of.push_back(i); }
        std::vector<std::pair<std::pair<uint32_t, unsigned long long>, uint32_t> > rec;
        for (int i = 0; i < n; i++) {
            if (has_pre_record(L.flags[i])) rec.push_back({{set_of(L, i), L.pre[i]}, (uint32_t)i << 1});
            if (has_post_record(L.flags[i])) rec.push_back({{set_of(L, i), L.post[i]}, ((uint32_t)i << 1) | 1u});
        }
        std::sort(rec.begin(), rec.end());
        rec_set.resize(rec.size()); rec_key.resize(rec.size()); rec_val.resize(rec.size());
        for (size_t r = 0; r < rec.size(); r++) { rec_set[r] = rec[r].first.first; rec_key[r] = rec[r].first.second; rec_val[r] = rec[r].second; }
        first_pre.assign((size_t)n, 0); first_post.assign((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            first_pre[(size_t)i] = first_record(rec_set.data(), rec_key.data(), (uint32_t)rec.size(), set_of(L, i), L.pre[i]);
            first_post[(size_t)i] = first_record(rec_set.data(), rec_key.data(), (uint32_t)rec.size(), set_of(L, i), L.post[i]);
        }
        L.node_of = node_of.data(); L.item_of = item_of.data();
        L.n_rec = (uint32_t)rec.size(); L.rec_set = rec_set.data(); L.rec_key = rec_key.data(); L.rec_val = rec_val.data();
        L.first_pre = first_pre.data(); L.first_post = first_post.data();
    }
};

// The walk by waves and rounds, the device behind two callables as in frontier._walk: gates(items, vbf) fills vbf[3 k ..] with the
// counts of refined candidate items[k] from the maps as they are; apply(ops, any_event) enters a wave's accepted candidates and
// applied events, `ops` in queue order.  A round decides from the states the round before left (what the kernels may see at the
// least).  stage is in/out (preset per candidate); counts [n][3], accepted, wave (1-based, the wave that decided the item) are
// written for every item.  rounds: per wave, when asked for.  Returns false when a round decides nothing or the waves exceed n
// (cannot be: the first undecided item always decides).
template <class Gates, class Apply>
inline bool walk_by_rounds(const Level& L, const int32_t* n_images, int32_t* stage, int32_t* counts, uint8_t* accepted, int32_t* wave,
                           int32_t* n_waves, std::vector<int>* rounds, Gates gates, Apply apply) {
    const size_t n = (size_t)L.n;
    std::vector<uint8_t> st(n, kUndecided), seen;
    for (size_t i = 0; i < n; i++) { counts[3 * i] = counts[3 * i + 1] = counts[3 * i + 2] = -1; accepted[i] = 0; wave[i] = 0; }
    *n_waves = 0;
    std::vector<int> pending, todo, ops;
    std::vector<int32_t> vbf, slot(n, -1);
    for (int w = 1;; w++) {
        pending.clear(); todo.clear(); ops.clear();
        for (size_t i = 0; i < n; i++) {
            st[i] = next_wave_state(st[i]);
            if (st[i] != kUndecided) continue;
            pending.push_back((int)i);
            if (!is_event(L.flags[i]) && (L.flags[i] & kRefined)) { slot[i] = (int32_t)todo.size(); todo.push_back((int)i); }
        }
        if (pending.empty()) return true;
        if ((size_t)w > n) return false;
        *n_waves = w;
        vbf.assign(3 * todo.size(), 0);
        if (!todo.empty()) gates(todo, vbf);
        size_t left = pending.size();
        int r = 0;
        while (left) {
            seen = st;
            size_t decided = 0;
            for (int i : pending) {
                if (seen[(size_t)i] != kUndecided) continue;
                const bool cand = !is_event(L.flags[i]) && (L.flags[i] & kRefined);
                const int32_t* g = cand ? &vbf[3 * (size_t)slot[(size_t)i]] : nullptr;
                Outcome o;
                if (!decide(L, seen.data(), i, g ? g[0] : 0, g ? g[1] : 0, g ? g[2] : 0, cand ? n_images[i] : 1, o)) continue;
                st[(size_t)i] = o.state;
                if (o.stage >= 0) stage[i] = o.stage;
                for (int k = 0; k < 3; k++) counts[3 * (size_t)i + k] = o.counts ? g[k] : -1;
                wave[i] = w;
                if (o.state == kAccept) accepted[i] = 1;
                decided++;
            }
            r++;
            if (!decided) return false;
            left -= decided;
        }
        if (rounds) rounds->push_back(r);
        bool any_event = false;
        for (int i : pending)
            if (st[(size_t)i] == kAccept || st[(size_t)i] == kApply) { ops.push_back(i); any_event |= st[(size_t)i] == kApply; }
        if (!ops.empty()) apply(ops, any_event);
    }
}

}  // namespace level_walk
