// octree.hpp -- the scheduler's DynOctTree as two key sets, and the look-ups CellProcessor::extend makes in it (reference
// src/hpmvs/CellProcessor.cpp:122-125, 147-154, include/hpmvs/doctree.h:250-255, 397-419, src/hpmvs/doctree.cpp:30-42).  Written
// once for the device kernels (kernel_octree.hip, kernel_octree_insert.hip) and for the host restatements the tests compile with
// g++ (tests/octree_host.cpp, tests/octree_insert_host.cpp).  DESIGN.md §3.11 has the argument; §3.12 the one for inserting a
// round's border patches in queue order (the second part of this file), §3.14 the one for the split into subtrees, §3.15 the one
// for a forest of subtrees behind one table buffer, §3.16 the one for the regularize / settle sweep over a forest, §3.17 the one
// for a round's border queue delivered to a forest (the last).
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
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
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

// ---- the two look-ups CellProcessor::extend makes per candidate (CellProcessor.cpp:122-125 before optimize, :147-154 after),
// against the tree as the level finds it.  `width` is the level's leaf width, add_width = extend_add_width(width).
struct ExtendPre {
    bool inside;        // getRoot()->contains(p)
    bool skip;          // inside, and the leaf at p is nonempty or narrower than `width` (:124): the candidate is never refined
    uint64_t pre_key;   // inside: addConditional's target at add_width, 0 where it refuses; outside: 0
};
HPMVS_OT_FN ExtendPre extend_pre(const Cell& root, const Table& t, const float* p, float width, float add_width) {
    ExtendPre r;
    r.inside = contains(root, p);
    r.skip = false;
    r.pre_key = 0;
    if (!r.inside) return r;
    const Located l = locate(root, t, p);
    r.skip = l.index != kAbsent || l.cell.w < width;
    r.pre_key = add_target(l, p, add_width);
    return r;
}
struct ExtendPost {
    bool border;        // !getRoot()->contains(p) (:147): handed to borderCellFn_
    uint64_t post_key;  // not border: addConditional's target, 0 where it refuses; border: 0
};
HPMVS_OT_FN ExtendPost extend_post(const Cell& root, const Table& t, const float* p, float add_width) {
    ExtendPost r;
    r.border = !contains(root, p);
    r.post_key = r.border ? 0 : add_target(locate(root, t, p), p, add_width);
    return r;
}
// cell->width_ * 0.9: a double product, narrowed by addConditional's float parameter
HPMVS_OT_FN float extend_add_width(float width) { return (float)((double)width * 0.9); }
// the depth d >= 1 whose cells have width_ == width under the root (the chain Cell(parent, idx) makes), -1 when there is none
HPMVS_OT_FN int level_depth(float root_width, float width) {
    float w = root_width;
    int d = 0;
    while (w > width && d < kMaxDepth) {
        w = (float)((double)w / 2.0);
        d++;
    }
    return (w == width && d >= 1) ? d : -1;
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

// ---- the split into subtrees (getSubTrees, reference src/main.cpp:50-96; DynOctTree::getSubTrees, doctree.h:513-523;
// Branch::nrLeafs, doctree.h:236-247).  The aligned key of a cell -- its path bits without the sentinel, shifted
// to the top of 63 bits -- orders cells as Leaf_iterator visits them (children 0 .. 7, depth first), and the cells below a key
// of depth d are the aligned keys in [align(key), align(key) + 8^(kMaxDepth - d)).  The nonempty leaves are prefix-free, so
// their aligned keys are distinct, and sorted ascending they ARE the Leaf_iterator order: the leaves of any subtree are one
// contiguous range of that order, and nrLeafs of any cell is two binary searches in it.
constexpr int kMaxSubtrees = 4096;                     // HPMVS_MAX_SUBTREES: the largest min_trees
constexpr int kMaxSubtreeList = kMaxSubtrees + 7;      // the list while it is cut: below min_trees, minus one, plus eight
constexpr int kStopRoot = 0, kStopEnough = 1, kStopSmall = 2;   // hpmvs_octree_partition_info::stop

HPMVS_OT_FN uint64_t aligned_key(uint64_t key) {
    const int d = key_depth(key);
    return (key ^ (1ull << (3 * d))) << (3 * (kMaxDepth - d));
}
HPMVS_OT_FN uint64_t aligned_span(uint64_t key) { return 1ull << (3 * (kMaxDepth - key_depth(key))); }
// the first position of the ascending a[0 .. n - 1] whose entry is not below v
HPMVS_OT_FN int32_t lower_bound(const uint64_t* a, int32_t n, uint64_t v) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the range of a cell's nonempty leaves in the sorted aligned leaf keys: its first position, and Branch::nrLeafs
HPMVS_OT_FN int32_t first_leaf(const uint64_t* sorted, int32_t n, uint64_t key) { return lower_bound(sorted, n, aligned_key(key)); }
HPMVS_OT_FN int32_t nr_leafs(const uint64_t* sorted, int32_t n, uint64_t key) {
    const uint64_t lo = aligned_key(key);
    return lower_bound(sorted, n, lo + aligned_span(key)) - lower_bound(sorted, n, lo);
}
// child idx of a cut cell: true when it is a BRANCH (it becomes a subtree, empty or not; a LEAF child enters none), *count its
// nrLeafs -- computed once, here: no subtree changes while the list is cut
HPMVS_OT_FN bool split_child(const Table& t, const uint64_t* sorted, int32_t n, uint64_t picked, unsigned idx, uint64_t* key, int32_t* count) {
    *key = (picked << 3) | idx;
    *count = nr_leafs(sorted, n, *key);
    return find(t, *key) == kBranch;
}
// main.cpp:67-75 as a maximum: the larger count first, then the LOWER list index (nrLeafs > maxLeafs is strict).  0 is below
// every entry: maxLeafs = -1 of the empty list.
HPMVS_OT_FN uint64_t split_rank(int32_t count, uint32_t index) { return ((uint64_t)(uint32_t)(count + 1) << 32) | (uint64_t)(0xffffffffu - index); }
HPMVS_OT_FN int32_t rank_count(uint64_t rank) { return (int32_t)(rank >> 32) - 1; }
HPMVS_OT_FN uint32_t rank_index(uint64_t rank) { return 0xffffffffu - (uint32_t)rank; }
// where entry i of the list goes when entry m is replaced by its n_new branch children, which come FIRST (main.cpp:81-88)
HPMVS_OT_FN int32_t split_position(int32_t i, int32_t m, int32_t n_new) { return i < m ? i + n_new : i + n_new - 1; }
// the cell of a key by the chain Cell(parent, idx) from the root
HPMVS_OT_FN Cell key_cell(const Cell& root, uint64_t key) {
    Cell b = root;
    for (int d = key_depth(key) - 1; d >= 0; d--) b = child(b, (unsigned)(key >> (3 * d)) & 7u);
    return b;
}
// a key re-based on its ancestor of depth root_depth: the sentinel, then the bits below that depth
HPMVS_OT_FN uint64_t sub_key(uint64_t key, int root_depth) {
    const int below = 3 * (key_depth(key) - root_depth);
    return (1ull << below) | (key & ((1ull << below) - 1));
}
// the subtree a key lies in: the value of the PROPER ancestor that is in `roots` (key -> list index; the final roots never
// nest, so at most one is), -1 when none is -- an orphan leaf, a root itself, or a branch above the roots
HPMVS_OT_FN int32_t owner_tree(const Table& roots, uint64_t key, int* root_depth) {
    int d = key_depth(key);
    for (uint64_t a = key >> 3; a != 0; a >>= 3) {
        d--;
        const int32_t v = find(roots, a);
        if (v >= 0) { *root_depth = d; return v; }
    }
    *root_depth = 0;
    return -1;
}

struct Split {
    int32_t n_trees, n_splits, stop;
};
// getSubTrees(tree, list, min_trees) on one thread, over the table and the sorted aligned keys of the nl nonempty leaves.
// list_key / list_count: [max(8, min_trees + 6)], the subtree roots in the reference's list order and their nrLeafs.
// min_split_leaves: the reference's 100 (main.cpp:78).  The loop ends: every cut takes one branch out of the list for good.
inline Split partition_sequential(const Table& t, const uint64_t* sorted, int32_t nl, int min_trees, int min_split_leaves,
                                  uint64_t* list_key, int32_t* list_count) {
    Split r{1, 0, kStopRoot};
    list_key[0] = kRootKey;
    list_count[0] = nl;
    if (min_trees < 2) return r;
    uint64_t rank = split_rank(list_count[0], 0);   // "do a first split", whatever the root holds
    while (true) {
        const int32_t m = (int32_t)rank_index(rank);
        uint64_t new_key[8];
        int32_t new_count[8], n_new = 0;
        for (unsigned idx = 0; idx < 8; idx++)
            if (split_child(t, sorted, nl, list_key[m], idx, &new_key[n_new], &new_count[n_new])) n_new++;
        std::vector<uint64_t> key(list_key, list_key + r.n_trees);
        std::vector<int32_t> count(list_count, list_count + r.n_trees);
        for (int32_t i = 0; i < r.n_trees; i++)
            if (i != m) { list_key[split_position(i, m, n_new)] = key[i]; list_count[split_position(i, m, n_new)] = count[i]; }
        for (int32_t k = 0; k < n_new; k++) { list_key[k] = new_key[k]; list_count[k] = new_count[k]; }
        r.n_trees += n_new - 1;
        if (r.n_trees >= min_trees) { r.stop = kStopEnough; return r; }
        rank = 0;
        for (int32_t i = 0; i < r.n_trees; i++) {
            const uint64_t x = split_rank(list_count[i], (uint32_t)i);
            if (x > rank) rank = x;
        }
        if (rank_count(rank) < min_split_leaves) { r.stop = kStopSmall; return r; }
        r.n_splits++;
    }
}

// ---- a forest: the subtrees of one priority level behind ONE table buffer (hpmvs_extend_forest_batch).  The
// trees' keys come concatenated (tree k's are [first[k], first[k + 1])), every key relative to its own tree's root.  Tree k owns
// the slot range [slot_first[k], slot_first[k] + table_slots(its keys)) of the buffer, so equal keys of different trees never
// meet and find / locate / extend_pre / extend_post work on a tree's Table as they do on a lone one.
struct Tree {
    Cell root;
    Table t;
};
// the first slot of every tree, [n_trees + 1]; the last entry is the size of the buffer in slots
inline void forest_slots(int32_t n_trees, const int32_t* branch_first, const int32_t* leaf_first, uint64_t* slot_first) {
    slot_first[0] = 0;
    for (int32_t k = 0; k < n_trees; k++)
        slot_first[k + 1] = slot_first[k] + table_slots((size_t)(branch_first[k + 1] - branch_first[k]) + (size_t)(leaf_first[k + 1] - leaf_first[k]));
}
// offsets as the call takes them: [n_trees + 1], from 0, non-decreasing.  -1 when they are, else the first tree whose range is bad
inline int32_t forest_offsets_bad(int32_t n_trees, const int32_t* first) {
    if (first[0] != 0) return 0;
    for (int32_t k = 0; k < n_trees; k++)
        if (first[k + 1] < first[k]) return k;
    return -1;
}
// the tree that owns entry i of a concatenated array: the LAST k with first[k] <= i (trees without keys own nothing)
HPMVS_OT_FN int32_t tree_of(const int32_t* first, int32_t n_trees, int32_t i) {
    int32_t lo = 0, hi = n_trees;   // first[lo] <= i < first[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// The verdict of a forest is ONE word folded with min: the lowest offending tree, and of that tree the finding a lone table's
// verdict would report first (key, then twice, then orphan).  kForestGood is above every finding.
constexpr uint32_t kForestGood = 0xffffffffu;
HPMVS_OT_FN uint32_t forest_finding(int32_t tree, int bad) {
    return ((uint32_t)tree << 2) | ((bad & kBadKey) ? 0u : (bad & kBadTwice) ? 1u : 2u);
}
HPMVS_OT_FN int32_t finding_tree(uint32_t v) { return (int32_t)(v >> 2); }
HPMVS_OT_FN int finding_bad(uint32_t v) { return 1 << (v & 3u); }
// entry i of the forest's keys, branches first: i < nb is branch_key[i], else leaf_key[i - nb]
struct ForestKey {
    uint64_t key;
    int32_t tree, index;   // index: of a leaf among its own tree's leaf keys (the table value), kBranch for a branch
};
HPMVS_OT_FN ForestKey forest_key(int32_t n_trees, const int32_t* branch_first, const int32_t* leaf_first, const uint64_t* branch_key,
                                 const uint64_t* leaf_key, int32_t i) {
    const int32_t nb = branch_first[n_trees];
    ForestKey r;
    if (i < nb) {
        r.key = branch_key[i];
        r.tree = tree_of(branch_first, n_trees, i);
        r.index = kBranch;
    } else {
        r.key = leaf_key[i - nb];
        r.tree = tree_of(leaf_first, n_trees, i - nb);
        r.index = i - nb - leaf_first[r.tree];
    }
    return r;
}
// the check of one key against the finished tables: kForestGood, or its finding
HPMVS_OT_FN uint32_t forest_check_key(const Tree* trees, const ForestKey& k) {
    if (key_form(k.key, k.index == kBranch)) return kForestGood;   // (reported by the build; its parent prefix means nothing)
    const int bad = key_parentage(trees[k.tree].t, k.key);
    return bad ? forest_finding(k.tree, bad) : kForestGood;
}
// The forest's device block, the same for every entry point that takes a forest:
//   [verdict words] [Tree x n_trees] [branch_first] [leaf_first] [extra] | [keys] [vals] | end
// every region at a multiple of 256 bytes.  Up to o_keys it is the header, which the host fills and ONE upload carries; `extra`
// are header bytes of the caller's own (the extend level's has_level); behind `end` the caller appends what is its own.  The
// verdict words are folded with min, each set to kForestGood before: kForestTable is the tables' finding, the others are the
// entry point's.  n_trees == 0 gives a block without tables and reads neither offset array.
constexpr int kForestTable = 0, kForestParent = 1, kForestLevel = 2, kForestWords = 4;
struct ForestBlock {
    size_t o_verdict, o_trees, o_bf, o_lf, o_extra, o_keys, o_vals, end;
    size_t slots;                       // of the whole buffer: slot_first[n_trees]
    std::vector<uint64_t> slot_first;   // [n_trees + 1]
};
inline ForestBlock forest_block(int32_t n_trees, const int32_t* branch_first, const int32_t* leaf_first, size_t extra_bytes) {
    const auto align = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t T = (size_t)n_trees;
    ForestBlock b;
    b.slot_first.assign(T + 1, 0);
    if (n_trees > 0) forest_slots(n_trees, branch_first, leaf_first, b.slot_first.data());
    b.slots = (size_t)b.slot_first[T];
    b.o_verdict = 0;
    b.o_trees = align(sizeof(uint32_t) * kForestWords);
    b.o_bf = align(b.o_trees + sizeof(Tree) * T);
    b.o_lf = align(b.o_bf + 4 * (T + 1));
    b.o_extra = align(b.o_lf + 4 * (T + 1));
    b.o_keys = align(b.o_extra + extra_bytes);
    b.o_vals = align(b.o_keys + 8 * b.slots);
    b.end = align(b.o_vals + 4 * b.slots);
    return b;
}
// the header's host image, hdr[0, o_keys), for a block that lies at the device address `base`; roots: [n_trees][4].  The extra
// bytes are zeroed.
inline void forest_block_fill(const ForestBlock& b, int32_t n_trees, const float* roots, const int32_t* branch_first,
                              const int32_t* leaf_first, uintptr_t base, char* hdr) {
    std::memset(hdr, 0, b.o_keys);
    for (int v = 0; v < kForestWords; v++) ((uint32_t*)(hdr + b.o_verdict))[v] = kForestGood;
    Tree* trees = (Tree*)(hdr + b.o_trees);
    for (int32_t k = 0; k < n_trees; k++) {
        const float* r = roots + 4 * (size_t)k;
        trees[k].root = Cell{{r[0], r[1], r[2]}, r[3]};
        trees[k].t = Table{(const uint64_t*)(base + b.o_keys + 8 * b.slot_first[k]), (const int32_t*)(base + b.o_vals + 4 * b.slot_first[k]),
                           (uint32_t)(b.slot_first[k + 1] - b.slot_first[k])};
    }
    if (n_trees > 0) {
        std::memcpy(hdr + b.o_bf, branch_first, 4 * ((size_t)n_trees + 1));
        std::memcpy(hdr + b.o_lf, leaf_first, 4 * ((size_t)n_trees + 1));
    }
}
// the two look-ups of a candidate through its tree's id
HPMVS_OT_FN ExtendPre extend_forest_pre(const Tree* trees, int32_t tree, const float* p, float width, float add_width) {
    return extend_pre(trees[tree].root, trees[tree].t, p, width, add_width);
}
HPMVS_OT_FN ExtendPost extend_forest_post(const Tree* trees, int32_t tree, const float* p, float add_width) {
    return extend_post(trees[tree].root, trees[tree].t, p, add_width);
}
// The build and the check on one thread (the device enters keys with a compare-and-swap, one lane per key): keys / vals are the
// table buffer of slot_first[n_trees] entries, keys zeroed; trees[k].t is pointed at tree k's range.  Returns the verdict word.
inline uint32_t forest_build_sequential(int32_t n_trees, const float* roots, const int32_t* branch_first, const int32_t* leaf_first,
                                        const uint64_t* branch_key, const uint64_t* leaf_key, const uint64_t* slot_first, uint64_t* keys,
                                        int32_t* vals, Tree* trees) {
    for (int32_t k = 0; k < n_trees; k++) {
        trees[k].root = Cell{{roots[4 * k], roots[4 * k + 1], roots[4 * k + 2]}, roots[4 * k + 3]};
        trees[k].t = Table{keys + slot_first[k], vals + slot_first[k], (uint32_t)(slot_first[k + 1] - slot_first[k])};
    }
    uint32_t verdict = kForestGood;
    const int32_t n = n_trees > 0 ? branch_first[n_trees] + leaf_first[n_trees] : 0;
    for (int32_t i = 0; i < n; i++) {
        const ForestKey k = forest_key(n_trees, branch_first, leaf_first, branch_key, leaf_key, i);
        uint32_t v = kForestGood;
        if (const int form = key_form(k.key, k.index == kBranch)) v = forest_finding(k.tree, form);
        else if (!insert(keys + slot_first[k.tree], vals + slot_first[k.tree], trees[k.tree].t.slots, k.key, k.index)) v = forest_finding(k.tree, kBadTwice);
        if (v < verdict) verdict = v;
    }
    for (int32_t i = 0; i < n; i++) {
        const uint32_t v = forest_check_key(trees, forest_key(n_trees, branch_first, leaf_first, branch_key, leaf_key, i));
        if (v < verdict) verdict = v;
    }
    return verdict;
}

// ---- one regularize / settle sweep of processCell over a forest, in queue order (hpmvs_process_forest_batch, reference
// CellProcessor.cpp:309-420).  A leaf changes at most once per sweep, and only its own cell changes it, so the
// tree as it stands at queue position q is the tree of the call plus ONE word per nonempty leaf -- the row of the cell that owns
// it -- and that row's decision: removed (the leaf is empty from then on) or split (it is a branch whose nonempty children are
// named by child_key).  Children born in the sweep are reachable only through their split parent: nothing enters the tables.
constexpr int32_t kNoOwner = 0x7fffffff;   // a leaf no cell of the sweep owns
HPMVS_OT_FN bool process_regularized(float flatness) { return flatness < 0.0f; }            // :399 (NaN is settled)
HPMVS_OT_FN bool process_removed(float flatness) { return (double)flatness > 2.4; }          // :409, float against double
HPMVS_OT_FN bool process_split(bool removed, int32_t support, bool final_level, int n_children) {   // branch, :221-224, :265-266
    return !removed && support >= 1 && !(final_level && n_children == 0);
}
// the leaf a child of a split cell goes into: Branch::at of the new branch
HPMVS_OT_FN uint64_t process_child_key(uint64_t cell_key, const Cell& cell, const float* p) { return (cell_key << 3) | octant(cell, p); }
// setDepths calls of one cell, in order: the cell's patch with subtract (removed or split), then a split cell's children in k order
HPMVS_OT_FN int process_op_count(bool removed, bool split, int n_children) { return removed ? 1 : split ? 1 + n_children : 0; }
// what the cell kernel finds wrong with a row, folded with min as (row << 3 | kind): the lowest row first
constexpr uint32_t kCellTree = 0, kCellLeaf = 1, kCellTwice = 2, kCellDeep = 3, kCellRef = 4;
HPMVS_OT_FN uint32_t cell_finding(int32_t row, uint32_t kind) { return ((uint32_t)row << 3) | kind; }

struct Sweep {
    const int32_t* owner;        // [all leaves of the forest] the row that owns the leaf, kNoOwner
    const uint8_t* removed;      // [n]
    const uint8_t* split;        // [n]
    const uint8_t* children;     // [n][4]
    const uint64_t* child_key;   // [n][4]
};
struct Probe {
    uint64_t key;      // of the leaf the probe ends in
    int32_t leaf;      // its index among ALL leaves of the forest when it is a nonempty leaf of the call's tree, else kAbsent
    int32_t child;     // row 4 j + k of the children when it is a leaf born in this sweep, else -1
};
// ptree->at(p) in the tree as it stands at queue position q; leaf_base = leaf_first[tree]
HPMVS_OT_FN Probe locate_versioned(const Tree& tr, int32_t leaf_base, const Sweep& s, int32_t q, const float* p) {
    const Located l = locate(tr.root, tr.t, p);
    Probe r{l.key, kAbsent, -1};
    if (l.index < 0) return r;   // (an empty leaf; kBranch: a branch at depth 21 cannot be in a checked table)
    const int32_t g = leaf_base + l.index, j = s.owner[g];
    if (j >= q) { r.leaf = g; return r; }              // untouched so far (kNoOwner is above every q)
    if (s.removed[j]) return r;
    if (!s.split[j]) { r.leaf = g; return r; }
    r.key = process_child_key(l.key, l.cell, p);        // one more step of Branch::at
    for (int k = 0; k < 4; k++)
        if (s.children[4 * (size_t)j + k] && s.child_key[4 * (size_t)j + k] == r.key) { r.child = 4 * j + k; return r; }
    return r;
}

// CellProcessor::regularize's arithmetic (:318-366), float as the reference's Eigen expressions evaluate
HPMVS_OT_FN float ot_dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
HPMVS_OT_FN void ot_cross3(const float* a, const float* b, float* r) {
    const float r0 = a[1] * b[2] - a[2] * b[1], r1 = a[2] * b[0] - a[0] * b[2], r2 = a[0] * b[1] - a[1] * b[0];
    r[0] = r0; r[1] = r1; r[2] = r2;
}
HPMVS_OT_FN void ot_normalized3(const float* a, float* r) {
    const float n2 = ot_dot3(a, a);
    if (n2 > 0.0f) { const float n = sqrtf(n2); r[0] = a[0] / n; r[1] = a[1] / n; r[2] = a[2] / n; }
    else { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; }
}
// probe `lane` of 24 (yy outer, xx inner, (0, 0) left out) of the patch (x0, normal pn) whose reference view has the x axis cam_x
HPMVS_OT_FN void regularize_probe(const float* x0, const float* pn, const float* cam_x, float width, int lane, float* p) {
    float t0[3], yaxis[3], xaxis[3];
    ot_cross3(pn, cam_x, t0);
    ot_normalized3(t0, yaxis);
    ot_cross3(yaxis, pn, xaxis);
    const int k = lane < 12 ? lane : lane + 1;
    const float fy = (float)(k / 5 - 2), fx = (float)(k % 5 - 2);
    for (int j = 0; j < 3; j++) p[j] = x0[j] + (fx * xaxis[j] + fy * yaxis[j]) * width;
}
// the squared plane distance of a neighbour's data[0]->center_ (nn: the normalized normal)
HPMVS_OT_FN float regularize_err2(const float* nn, const float* x0, const float* pc) {
    const float b[3] = {pc[0] - x0[0], pc[1] - x0[1], pc[2] - x0[2]};
    const float e = ot_dot3(nn, b);
    return e * e;
}
HPMVS_OT_FN float regularize_flatness(int cnt, float dist, float width) {
    if (cnt < 1) return 2.6f;
    if (cnt < 4) return 2.5f;
    return sqrtf(dist / (float)cnt) / width;
}

// The sweep on one thread: the host restatement the tests load, row by row as the reference's queue runs.  What the refinement
// decides is an input here: support [n], child_ok [n][4] (the child was built, refined and passed both gates), child_center
// [n][4][3].  cam_x: [n][3] the x axis of every cell's reference view.  ops: the setDepths calls in order, a cell's own patch as
// its row i, child k of cell i as n + 4 i + k; op_subtract beside it.  Returns kForestGood or the cell finding.
inline uint32_t process_sequential(int32_t n_trees, const Tree* trees, const int32_t* leaf_first, const float* leaf_patch_center, int32_t n,
                                   const float* center, const float* normal, const float* cam_x, const uint8_t* ref_ok,
                                   const int32_t* cell_tree, const uint64_t* cell_key, float* flatness, const uint8_t* final_level,
                                   const int32_t* support, const uint8_t* child_ok, const float* child_center, uint8_t* removed,
                                   uint8_t* split, uint8_t* children, uint64_t* child_key, int32_t* n_neighbours, uint64_t* neighbour_key,
                                   std::vector<int32_t>* ops, std::vector<uint8_t>* op_subtract) {
    std::vector<int32_t> owner(n_trees > 0 ? (size_t)leaf_first[n_trees] : 0, kNoOwner), gleaf((size_t)n, -1);
    uint32_t verdict = kForestGood;
    auto find_bad = [&](int32_t i, uint32_t kind) { if (cell_finding(i, kind) < verdict) verdict = cell_finding(i, kind); };
    for (int32_t i = 0; i < n; i++) {
        const int32_t k = cell_tree[i];
        if (k < 0 || k >= n_trees) { find_bad(i, kCellTree); continue; }
        const int32_t idx = key_depth(cell_key[i]) < 1 ? kAbsent : find(trees[k].t, cell_key[i]);
        if (idx < 0) { find_bad(i, kCellLeaf); continue; }
        gleaf[i] = leaf_first[k] + idx;
        if (owner[gleaf[i]] != kNoOwner) find_bad(i, kCellTwice); else owner[gleaf[i]] = i;
        const bool reg = process_regularized(flatness[i]);
        if (!reg && !process_removed(flatness[i]) && key_depth(cell_key[i]) >= kMaxDepth) find_bad(i, kCellDeep);
        if (reg && !ref_ok[i]) find_bad(i, kCellRef);
    }
    if (verdict != kForestGood) return verdict;
    const Sweep sw{owner.data(), removed, split, children, child_key};
    for (int32_t i = 0; i < n; i++) {
        removed[i] = split[i] = 0;
        for (int k = 0; k < 4; k++) { children[4 * (size_t)i + k] = 0; child_key[4 * (size_t)i + k] = 0; }
        for (int k = 0; k < 24; k++) neighbour_key[24 * (size_t)i + k] = 0;
        n_neighbours[i] = -2;
        const Tree& tr = trees[cell_tree[i]];
        const Cell cell = key_cell(tr.root, cell_key[i]);
        const float* x0 = center + 4 * (size_t)i;
        const float* pn = normal + 4 * (size_t)i;
        if (process_regularized(flatness[i])) {
            float nn[3], dist = 0.0f;
            ot_normalized3(pn, nn);
            int cnt = 0;
            for (int lane = 0; lane < 24; lane++) {
                float p[3];
                regularize_probe(x0, pn, cam_x + 3 * (size_t)i, cell.w, lane, p);
                const Probe pr = locate_versioned(tr, leaf_first[cell_tree[i]], sw, i, p);
                if (pr.leaf == kAbsent && pr.child < 0) continue;
                bool first = true;
                for (int j = 0; j < cnt && first; j++) first = neighbour_key[24 * (size_t)i + j] != pr.key;
                if (!first) continue;
                neighbour_key[24 * (size_t)i + cnt++] = pr.key;
                dist += regularize_err2(nn, x0, pr.child >= 0 ? child_center + 3 * (size_t)pr.child : leaf_patch_center + 3 * (size_t)pr.leaf);
            }
            n_neighbours[i] = cnt;
            flatness[i] = regularize_flatness(cnt, dist, cell.w);
            continue;
        }
        removed[i] = process_removed(flatness[i]) ? 1 : 0;
        int nc = 0;
        if (!removed[i] && support[i] >= 1)
            for (int k = 0; k < 4; k++)
                if (child_ok[4 * (size_t)i + k]) { children[4 * (size_t)i + k] = 1; nc++; }
        split[i] = process_split(removed[i] != 0, support[i], final_level[i] != 0, nc) ? 1 : 0;
        if (!split[i])
            for (int k = 0; k < 4; k++) children[4 * (size_t)i + k] = 0;   // (a final-level leaf without children keeps its patch)
        for (int k = 0; k < 4; k++)
            if (children[4 * (size_t)i + k]) child_key[4 * (size_t)i + k] = process_child_key(cell_key[i], cell, child_center + 3 * (4 * (size_t)i + k));
        if (process_op_count(removed[i] != 0, split[i] != 0, nc)) { ops->push_back(i); op_subtract->push_back(1); }
        if (split[i])
            for (int k = 0; k < 4; k++)
                if (children[4 * (size_t)i + k]) { ops->push_back(n + 4 * i + k); op_subtract->push_back(0); }
    }
    return kForestGood;
}

// ---- a round's border queue delivered to a forest (hpmvs_border_forest_batch, reference CellProcessor.cpp:487-540, DESIGN.md
// §3.17): distributeBorderCell hands patch i to the first tree in list order whose root contains center_, and every tree's
// processBorderCellQueue inserts what it was handed in queue order with addConditional(center_, scale_3dx_ * 2.0).  Trees never
// meet, so a run of the replay is a (tree, static leaf key) PAIR: two trees often hold the same sub-key.
// scale_3dx_ * 2.0: a double product, narrowed by addConditional's float parameter
HPMVS_OT_FN float border_add_width(float scale) { return (float)((double)scale * 2.0); }
// distributeBorderCell's search over the trees of a forest
HPMVS_OT_FN int32_t route(int32_t n_trees, const Tree* trees, const float* p) {
    for (int32_t k = 0; k < n_trees; k++)
        if (contains(trees[k].root, p)) return k;
    return -1;
}
// The queue on one thread: the route loop, then insert_sequential per tree over that tree's rows in their given order, the
// blocker mapped back through the row selection.  center: [n][4] as a patch batch holds it.  The host restatement the tests
// load, and the loop the one call's cost is set against.  tree / accepted / leaf_key: [n]; blocker: [n], nullable.
inline void border_forest_sequential(int32_t n_trees, const Tree* trees, int n, const float* center, const float* scale, int32_t* tree,
                                     uint8_t* accepted, uint64_t* leaf_key, int32_t* blocker) {
    std::vector<std::vector<int32_t>> rows(n_trees > 0 ? (size_t)n_trees : 0);
    for (int i = 0; i < n; i++) {
        tree[i] = route(n_trees, trees, center + 4 * (size_t)i);
        accepted[i] = 0;
        leaf_key[i] = 0;
        if (blocker) blocker[i] = -1;
        if (tree[i] >= 0) rows[(size_t)tree[i]].push_back(i);
    }
    for (int32_t k = 0; k < n_trees; k++) {
        const std::vector<int32_t>& sel = rows[(size_t)k];
        const int m = (int)sel.size();
        if (m == 0) continue;
        std::vector<float> pts(3 * (size_t)m), aw((size_t)m);
        std::vector<uint8_t> acc((size_t)m);
        std::vector<uint64_t> key((size_t)m);
        std::vector<int32_t> blk((size_t)m);
        for (int j = 0; j < m; j++) {
            for (int c = 0; c < 3; c++) pts[3 * (size_t)j + c] = center[4 * (size_t)sel[j] + c];
            aw[j] = border_add_width(scale[sel[j]]);
        }
        insert_sequential(trees[k].root, trees[k].t, m, pts.data(), aw.data(), acc.data(), key.data(), blk.data());
        for (int j = 0; j < m; j++) {
            accepted[sel[j]] = acc[j];
            leaf_key[sel[j]] = key[j];
            if (blocker) blocker[sel[j]] = blk[j] < 0 ? -1 : sel[blk[j]];
        }
    }
}

}  // namespace octree
}  // namespace hpmvs
