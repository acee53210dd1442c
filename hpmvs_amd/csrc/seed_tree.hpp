// seed_tree.hpp -- the octree Scene::initPatches builds from its surviving seeds (reference src/hpmvs/Scene.cpp:183-199),
// as a closed form of the sequential insertion.  Written once for the device kernels (kernel_seed_tree.hip) and for the host
// restatement the tests compile with g++ (tests/seed_tree_host.cpp).  DESIGN.md §3.10 has the argument.
//
//   getBoundingBox (doctree.h:732-756)   min starts at FLT_MAX, max at std::numeric_limits<float>::min() = FLT_MIN (so a cloud of
//                                        negative coordinates keeps max = FLT_MIN); std::min / std::max: a NaN never enters
//   root                                 Branch((min + max) / 2, max(dist)), float arithmetic; always a Branch: leaves start at depth 1
//   scale floor (Scene.cpp:196)          max(scale, width / (1 << PATCH_INIT_MAXLEVEL + 1)): + binds before <<
//   DynOctTree::add(e, width)            (doctree.h:379-394) descends to e's leaf and splits it while leaf width / 2.0 > width
//   Cell(parent, idx), Branch::at        (doctree.cpp:30-36, doctree.h:250-255) double arithmetic, float storage; child bit x > c_
//
// add() only ever splits.  Inserted alone, e stops at depth d(e): the smallest k >= 1 for which w_k / 2.0 > width(e) is false,
// w_k the root width halved k times.  A node at depth k of e's path ends as a Branch exactly when some element e' below it has
// d(e') > k, so e's final leaf lies at depth D(e) = max over e' of min(lcp(e, e') + 1, d(e')), lcp = common path levels.
// Build with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__)
#define HPMVS_ST_FN __host__ __device__ inline
#else
#define HPMVS_ST_FN inline
#endif

namespace hpmvs {
namespace seed {

constexpr int kMaxDepth = 21;                       // path levels of a key: 3 bits each, left-aligned in 63 bits
constexpr uint64_t kAbsent = (uint64_t)1 << 63;    // key of a row that takes no part (ok == 0): sorts behind every path

HPMVS_ST_FN uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
HPMVS_ST_FN float bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
// order-preserving integer image of a float (not NaN): a < b  <=>  ordered(a) < ordered(b); -0 lies below +0
HPMVS_ST_FN uint32_t ordered(float f) { const uint32_t u = float_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
HPMVS_ST_FN float unordered(uint32_t o) { return bits_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// one step of getBoundingBox's fold: std::min(min, x), std::max(max, x)
HPMVS_ST_FN void box_add(float* mn, float* mx, const float* p) {
    for (int k = 0; k < 3; k++) {
        mn[k] = p[k] < mn[k] ? p[k] : mn[k];
        mx[k] = mx[k] < p[k] ? p[k] : mx[k];
    }
}

struct Root {
    float c[3], w, floor;
    bool finite;
};
// the root Branch and the scale floor from the fold's result; no element: the unit cube of getBoundingBox
HPMVS_ST_FN Root make_root(const float* mn_in, const float* mx_in, int n_rows, int patch_init_maxlevel) {
    float mn[3], mx[3], dist[3];
    for (int k = 0; k < 3; k++) {
        mn[k] = n_rows > 0 ? mn_in[k] : -1.0f;
        mx[k] = n_rows > 0 ? mx_in[k] : 1.0f;
        dist[k] = mx[k] - mn[k];
    }
    Root r;
    const float inner = dist[1] < dist[2] ? dist[2] : dist[1];
    r.w = dist[0] < inner ? inner : dist[0];
    for (int k = 0; k < 3; k++) r.c[k] = (mn[k] + mx[k]) / 2.0f;
    r.floor = r.w / (float)(1 << (patch_init_maxlevel + 1));
    r.finite = true;
    for (int k = 0; k < 3; k++) r.finite = r.finite && r.c[k] - r.c[k] == 0.0f;
    r.finite = r.finite && r.w - r.w == 0.0f;
    return r;
}

// std::max(scale, floor): a NaN scale stays
HPMVS_ST_FN float floored(float scale, float floor) { return scale < floor ? floor : scale; }

// d(e).  The floor makes it <= max(1, PATCH_INIT_MAXLEVEL) for any root width whose halvings are exact; the bound only acts on
// subnormal widths, where the reference would go on splitting cells of width 0.
HPMVS_ST_FN int depth_alone(float root_width, float width) {
    float w = root_width;
    int k = 0;
    do {
        w = (float)((double)w / 2.0);
        k++;
    } while (k < kMaxDepth && (double)w / 2.0 > (double)width);
    return k;
}

HPMVS_ST_FN unsigned octant(const float* c, const float* p) {
    return ((unsigned)(p[2] > c[2]) << 2) | ((unsigned)(p[1] > c[1]) << 1) | (unsigned)(p[0] > c[0]);
}
// Cell(parent, idx) of the child that holds p
HPMVS_ST_FN void child(float* c, float& w, const float* p) {
    const float cw = (float)((double)w / 2.0);
    for (int k = 0; k < 3; k++) c[k] = (float)((double)c[k] + ((p[k] > c[k]) ? 1.0 : -1.0) * (double)cw / 2.0);
    w = cw;
}
// the cell `levels` below the root on p's path
HPMVS_ST_FN void descend(const Root& r, const float* p, int levels, float* c, float& w) {
    c[0] = r.c[0]; c[1] = r.c[1]; c[2] = r.c[2];
    w = r.w;
    for (int k = 0; k < levels; k++) child(c, w, p);
}
HPMVS_ST_FN uint64_t path_key(const Root& r, const float* p) {
    float c[3] = {r.c[0], r.c[1], r.c[2]};
    float w = r.w;
    uint64_t key = 0;
    for (int k = 0; k < kMaxDepth; k++) {
        key = (key << 3) | octant(c, p);
        child(c, w, p);
    }
    return key;
}
// common path levels of two keys
HPMVS_ST_FN int lcp(uint64_t a, uint64_t b) { return a == b ? kMaxDepth : (__builtin_clzll(a ^ b) - 1) / 3; }
// the first `depth` levels of a key, left-aligned: leaves are disjoint, so the padded prefixes order them as Leaf_iterator does
HPMVS_ST_FN uint64_t leaf_key(uint64_t key, int depth) { return key & ~((((uint64_t)1) << (3 * (kMaxDepth - depth))) - 1); }

// x -> min(hi, max(lo, x)) with lo <= hi.  With the elements sorted by key, lcp(i, j) is the minimum of the adjacent lcps between
// them, so R[i] = max over j > i of min(lcp(i, j) + 1, d[j]) = min(L[i] + 1, max(d[i + 1], R[i + 1])): a chain of clamps applied to
// 0, and clamps compose into clamps -- one associative scan per side.
struct Clamp {
    int32_t lo, hi;
};
HPMVS_ST_FN int32_t clamp_apply(const Clamp& c, int32_t x) { return x < c.lo ? c.lo : (x > c.hi ? c.hi : x); }
// x -> min(a, max(b, x))
HPMVS_ST_FN Clamp clamp_make(int32_t a, int32_t b) { return Clamp{b < a ? b : a, a}; }
// first, then second
HPMVS_ST_FN Clamp clamp_then(const Clamp& first, const Clamp& second) {
    return Clamp{clamp_apply(second, first.lo), clamp_apply(second, first.hi)};
}
struct ClampThen {
    HPMVS_ST_FN Clamp operator()(const Clamp& first, const Clamp& second) const { return clamp_then(first, second); }
};
// Position i of the key-sorted elements (n_rows of them).  Left chain, scanned in order: element i applies the step from i - 1 to
// i.  Right chain, scanned over t = n - 1 - i: element t applies the step from i + 1 to i.  Ends and absent rows: the constant 0.
HPMVS_ST_FN Clamp left_step(int i, int n_rows, int lcp_prev, int d_prev) {
    return (i == 0 || i >= n_rows) ? Clamp{0, 0} : clamp_make(lcp_prev + 1, d_prev);
}
HPMVS_ST_FN Clamp right_step(int i, int n_rows, int lcp_next, int d_next) {
    return i >= n_rows - 1 ? Clamp{0, 0} : clamp_make(lcp_next + 1, d_next);
}
HPMVS_ST_FN int final_depth(int d, const Clamp& left, const Clamp& right) {
    const int a = clamp_apply(left, 0), b = clamp_apply(right, 0);
    const int m = a > b ? a : b;
    return d > m ? d : m;
}

}  // namespace seed
}  // namespace hpmvs
