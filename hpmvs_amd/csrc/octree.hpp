// octree.hpp -- the scheduler's DynOctTree as two key sets, and the look-ups CellProcessor::extend makes in it (reference
// src/hpmvs/CellProcessor.cpp:122-125, 147-154, include/hpmvs/doctree.h:250-255, 397-419, src/hpmvs/doctree.cpp:30-42).  Written
// once for the device kernels (kernel_octree.hip, kernel_octree_insert.hip) and for the host restatements the tests compile with
// g++ (tests/octree_host.cpp, tests/octree_insert_host.cpp).  DESIGN.md §3.11 has the argument; §3.12 the one for inserting a
// round's border patches in queue order (the second half of this file).
//
//   path key                 a sentinel bit, then 3 bits per level (z y x, Branch::at's child test x > c_): the root is 1, a cell
//                            at depth d has 3 d bits below the sentinel; at most kMaxDepth = 21 levels (kernel_regularize.hip's form)
//   the tree                 branch keys (the root is implicit) and the keys of the NONEMPTY leaves; an empty leaf is a key that is
//                            in neither set and whose parent is a branch
//   Cell(parent, idx)        width_ = parent width / 2.0, c_[k] = parent c_[k] +- width_ / 2.0: double arithmetic, float storage
//   Cell::contains           hw = width_ / 2.0 narrowed to float; p > c_ - hw below, p <= c_ + hw above, float arithmetic
//   Branch::at               descends whatever the point: one outside the root lands in a border leaf, a NaN coordinate takes bit 0
//   addConditional(e, w)     refuses on a nonempty leaf or one with width_ < w; else splits while width_ / 2.0 > w
// Build with -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define HPMVS_OT_FN __host__ __device__ inline
#else
#define HPMVS_OT_FN inline
#endif

namespace hpmvs {
namespace octree {

constexpr int kMaxDepth = 21;
constexpr uint64_t kRootKey = 1;
constexpr int32_t kBranch = -2;    // table value of a branch key; a nonempty leaf's is its index (>= 0)
constexpr int32_t kAbsent = -1;    // look-up of a key that is in neither set

struct Cell {
    float c[3], w;
};

HPMVS_OT_FN unsigned octant(const Cell& b, const float* p) {
    return ((unsigned)(p[2] > b.c[2]) << 2) | ((unsigned)(p[1] > b.c[1]) << 1) | (unsigned)(p[0] > b.c[0]);
}
// Cell(parent, idx)
HPMVS_OT_FN Cell child(const Cell& b, unsigned idx) {
    Cell r;
    r.w = (float)((double)b.w / 2.0);
    for (int k = 0; k < 3; k++) r.c[k] = (float)((double)b.c[k] + (((idx >> k) & 1u) ? 1.0 : -1.0) * (double)r.w / 2.0);
    return r;
}
HPMVS_OT_FN bool contains(const Cell& b, const float* p) {
    const float hw = (float)((double)b.w / 2.0);
    return p[0] > b.c[0] - hw && p[1] > b.c[1] - hw && p[2] > b.c[2] - hw && p[0] <= b.c[0] + hw && p[1] <= b.c[1] + hw &&
           p[2] <= b.c[2] + hw;
}

// levels of a key below the root; -1 for a word that is no key (0, or a sentinel off the 3-bit grid)
HPMVS_OT_FN int key_depth(uint64_t key) {
    if (key == 0) return -1;
    const int top = 63 - __builtin_clzll(key);
    return top % 3 == 0 ? top / 3 : -1;
}
HPMVS_OT_FN uint64_t key_parent(uint64_t key) { return key >> 3; }

// ---- the two key sets as ONE open-addressing table: key -> kBranch or the leaf's index.  A key can be entered once, which is
// what makes "twice in one set" and "branch and leaf at once" the same finding.
HPMVS_OT_FN uint64_t hash(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}
struct Table {
    const uint64_t* keys;   // [slots] 0 = free
    const int32_t* vals;    // [slots]
    uint32_t slots;         // a power of two, > the number of keys
};
HPMVS_OT_FN uint32_t table_slots(size_t n_keys) {
    uint32_t s = 2;
    while ((size_t)s < 2 * n_keys) s <<= 1;
    return s;
}
HPMVS_OT_FN int32_t find(const Table& t, uint64_t key) {
    const uint64_t mask = (uint64_t)t.slots - 1;
    uint64_t h = hash(key) & mask;
    while (true) {   // slots > keys: a free slot ends every chain
        const uint64_t k = t.keys[h];
        if (k == 0) return kAbsent;
        if (k == key) return t.vals[h];
        h = (h + 1) & mask;
    }
}
// sequential insertion (the host's; the device enters keys with a compare-and-swap): false when the key is there already
inline bool insert(uint64_t* keys, int32_t* vals, uint32_t slots, uint64_t key, int32_t val) {
    const uint64_t mask = (uint64_t)slots - 1;
    uint64_t h = hash(key) & mask;
    while (keys[h] != 0) {
        if (keys[h] == key) return false;
        h = (h + 1) & mask;
    }
    keys[h] = key;
    vals[h] = val;
    return true;
}

// What a table must satisfy, key by key (bits of the verdict).  A branch at depth 21 is refused with the deep keys: its children
// could not be named.
constexpr int kBadKey = 1;       // no key, the root, or deeper than kMaxDepth (a branch: deeper than kMaxDepth - 1)
constexpr int kBadTwice = 2;     // entered twice: a duplicate, or a branch that is also a leaf
constexpr int kBadOrphan = 4;    // its parent prefix is neither a branch nor the root
HPMVS_OT_FN int key_form(uint64_t key, bool branch) {
    const int d = key_depth(key);
    return (d < 1 || d > kMaxDepth - (branch ? 1 : 0)) ? kBadKey : 0;
}
HPMVS_OT_FN int key_parentage(const Table& t, uint64_t key) {
    const uint64_t par = key_parent(key);
    return (par == kRootKey || find(t, par) == kBranch) ? 0 : kBadOrphan;
}

struct Located {
    uint64_t key;       // of the leaf
    int32_t index;      // into the leaf table, kAbsent for an empty leaf
    Cell cell;          // its c_ / width_
};
// root->at(p): descend while the key is a branch; the first key that is not one is the leaf
HPMVS_OT_FN Located locate(const Cell& root, const Table& t, const float* p) {
    Located r;
    r.cell = root;
    r.key = kRootKey;
    r.index = kBranch;
    for (int d = 0; d < kMaxDepth && r.index == kBranch; d++) {
        const unsigned idx = octant(r.cell, p);
        r.key = (r.key << 3) | idx;
        r.cell = child(r.cell, idx);
        r.index = find(t, r.key);
    }
    return r;
}
// addConditional(p, add_width) from the located leaf: 0 when it refuses, else the key of the leaf the element ends in.  The
// depth bound only acts where the reference would go on splitting cells past 21 levels (add_width <= 0, subnormal widths).
HPMVS_OT_FN uint64_t add_target(const Located& leaf, const float* p, float add_width) {
    if (leaf.index != kAbsent || leaf.cell.w < add_width) return 0;
    Cell b = leaf.cell;
    uint64_t key = leaf.key;
    int d = key_depth(key);
    while (d < kMaxDepth && (double)b.w / 2.0 > (double)add_width) {
        const unsigned idx = octant(b, p);
        key = (key << 3) | idx;
        b = child(b, idx);
        d++;
    }
    return key;
}

// ---- a round's border patches, inserted in queue order (CellProcessor::processBorderCellQueue, CellProcessor.cpp:500-531): a
// loop of addConditional(p_i, a_i) with a width of its own per patch, so that an earlier insertion changes what a later one
// finds.  Against the tree as the round finds it:
//   static     L_i = root->at(p_i) in the unchanged tree; nonempty or narrower than a_i refuses whatever was inserted before
//              (insertions only split EMPTY leaves).  Everything an insertion creates lies below its static leaf, so patches
//              with different static leaves never meet.
//   full path  the 21 octant choices of p_i down the nested Cell(parent, idx), whatever the table holds
//   dynamic    within one static leaf, A = the keys accepted so far: a prefix-free set, its proper prefixes below L are the
//              branches the splits made.  lcp_j = levels on which path_i and A_j agree.  lcp_j == depth(A_j): p_i descends into
//              the nonempty leaf A_j (at most one j; it holds the largest lcp).  Otherwise p_i finds the empty sibling at depth
//              f = max_j lcp_j + 1 (f = depth(L) while A is empty), and addConditional goes on from there.
struct Widths {
    float w[kMaxDepth + 1];   // width_ of every cell of a depth: the chain Cell(parent, idx) makes, the root's at [0]
};
HPMVS_OT_FN Widths level_widths(float root_width) {
    Widths r;
    r.w[0] = root_width;
    for (int d = 1; d <= kMaxDepth; d++) r.w[d] = (float)((double)r.w[d - 1] / 2.0);
    return r;
}
// the full path of a point: a key of depth kMaxDepth
HPMVS_OT_FN uint64_t full_path(const Cell& root, const float* p) {
    Cell b = root;
    uint64_t key = kRootKey;
    for (int d = 0; d < kMaxDepth; d++) {
        const unsigned idx = octant(b, p);
        key = (key << 3) | idx;
        b = child(b, idx);
    }
    return key;
}
HPMVS_OT_FN uint64_t path_prefix(uint64_t path, int depth) { return path >> (3 * (kMaxDepth - depth)); }
// levels on which a full path and the key `key` of depth `depth` agree (at most `depth`)
HPMVS_OT_FN int path_lcp(uint64_t path, uint64_t key, int depth) {
    const uint64_t x = path_prefix(path, depth) ^ key;   // (the sentinels cancel)
    return x == 0 ? depth : depth - 1 - (63 - __builtin_clzll(x)) / 3;
}

struct Inserted {
    uint64_t key;    // *outleaf: the leaf the patch went into, or the one that refused it
    int32_t depth;   // of that key
    bool accepted;
};
// addConditional(p, a) for a survivor of the static test, after the insertions A into its static leaf (of depth leaf_depth):
// `any` = A is not empty, max_lcp = max_j lcp_j, hit = that lcp is the whole of its key.  width = Widths::w.
HPMVS_OT_FN Inserted insert_decide(int leaf_depth, uint64_t path, float a, const float* width, bool any, int max_lcp, bool hit) {
    Inserted r;
    r.accepted = false;
    if (any && hit) {   // leaf->data nonempty
        r.depth = max_lcp;
        r.key = path_prefix(path, max_lcp);
        return r;
    }
    int d = any ? max_lcp + 1 : leaf_depth;
    r.depth = d;
    r.key = path_prefix(path, d);
    if (width[d] < a) return r;   // leaf->width_ < width
    while (d < kMaxDepth && (double)width[d] / 2.0 > (double)a) d++;
    r.depth = d;
    r.key = path_prefix(path, d);
    r.accepted = true;
    return r;
}
// one member against one accepted key, as the lanes of the replay kernel fold it with max: the longer lcp first, then the EARLIER
// position in A (the blocker of a "too narrow" refusal is the accepted patch with the longest lcp, lowest index on ties).  The
// hit bit rides below the lcp: a hit holds the strictly largest lcp of A, so it never decides an order.
HPMVS_OT_FN uint64_t lcp_rank(uint64_t path, uint64_t key, uint32_t pos) {
    const int depth = key_depth(key), lcp = path_lcp(path, key, depth);
    return ((uint64_t)(uint32_t)lcp << 33) | ((uint64_t)(lcp == depth) << 32) | (uint64_t)(0xffffffffu - pos);
}
HPMVS_OT_FN int rank_lcp(uint64_t rank) { return (int)(rank >> 33); }
HPMVS_OT_FN bool rank_hit(uint64_t rank) { return ((rank >> 32) & 1u) != 0; }
HPMVS_OT_FN uint32_t rank_pos(uint64_t rank) { return 0xffffffffu - (uint32_t)rank; }

// The loop itself on one thread: patch by patch in queue order, the accepted keys kept per static leaf.  The host restatement
// the tests load, and the loop the batched call's cost is set against.  accepted / leaf_key / blocker: [n], blocker nullable
// (-1 for an accepted patch and a static refusal, else the queue index of the earlier patch that caused the refusal).
inline void insert_sequential(const Cell& root, const Table& t, int n, const float* points, const float* add_width, uint8_t* accepted,
                              uint64_t* leaf_key, int32_t* blocker) {
    struct Entry { uint64_t key; int32_t owner; };
    std::unordered_map<uint64_t, std::vector<Entry>> runs;
    const Widths W = level_widths(root.w);
    for (int i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        const float a = add_width[i];
        const Located l = locate(root, t, p);
        accepted[i] = 0;
        leaf_key[i] = l.key;
        if (blocker) blocker[i] = -1;
        if (l.index != kAbsent || l.cell.w < a) continue;
        const uint64_t path = full_path(root, p);
        std::vector<Entry>& A = runs[l.key];
        uint64_t best = 0;
        for (size_t j = 0; j < A.size(); j++) {
            const uint64_t r = lcp_rank(path, A[j].key, (uint32_t)j);
            if (r > best) best = r;
        }
        const bool any = !A.empty();
        const Inserted r = insert_decide(key_depth(l.key), path, a, W.w, any, rank_lcp(best), rank_hit(best));
        accepted[i] = r.accepted ? 1 : 0;
        leaf_key[i] = r.key;
        if (r.accepted) A.push_back(Entry{r.key, i});
        else if (blocker && any) blocker[i] = A[rank_pos(best)].owner;
    }
}

}  // namespace octree
}  // namespace hpmvs
