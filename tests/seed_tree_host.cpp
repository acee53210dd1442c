// Host restatement of hpmvs_seed_tree_batch, steps 1-7 (include/hpmvs_amd.h): the product's arithmetic
// (hpmvs_amd/csrc/seed_tree.hpp) compiled by g++, with std::stable_sort and sequential scans in place of rocPRIM's.
// tests/test_cpu_seed_tree.py pins it to the sequential DynOctTree::add of tests/octree_ref.py; the GPU tests compare the
// kernels with it byte for byte.  Build: g++ -std=c++11 -O2 -ffp-contract=off -fPIC -shared seed_tree_host.cpp
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../hpmvs_amd/csrc/seed_tree.hpp"

using namespace hpmvs::seed;

extern "C" {

// info: root_center[3], root_width, scale_floor as floats, then n_rows, n_leaves as int32 (hpmvs_seed_tree_info).
// center [n][4], scale [n] in/out, ok [n] or null; outputs as hpmvs_seed_tree_batch, leaf_key [n] (nullable) the leaves' padded
// path prefixes.  Returns 0, or -2 for a root that is not finite (nothing written).
int st_seed_tree(int n, const float* center, float* scale, const uint8_t* ok, int patch_init_maxlevel, void* info, int32_t* rows,
                 int32_t* cell_start, float* cell_center, float* cell_width, int32_t* cell_level, float* patch_center,
                 uint64_t* leaf_keys) {
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {FLT_MIN, FLT_MIN, FLT_MIN};
    int n_rows = 0;
    for (int i = 0; i < n; i++)
        if (!ok || ok[i]) {
            box_add(mn, mx, center + 4 * (size_t)i);
            n_rows++;
        }
    const Root r = make_root(mn, mx, n_rows, patch_init_maxlevel);
    if (!r.finite) return -2;
    std::vector<uint64_t> key(n), lkey(n);
    std::vector<int32_t> d(n, 0), D(n, 0), order(n);
    for (int i = 0; i < n; i++) {
        key[i] = kAbsent;
        if (ok && !ok[i]) continue;
        scale[i] = floored(scale[i], r.floor);
        d[i] = depth_alone(r.w, scale[i]);
        key[i] = path_key(r, center + 4 * (size_t)i);
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
    std::vector<Clamp> left(n), right(n);
    for (int i = 0; i < n; i++) {
        const bool prev = i > 0 && i < n_rows, next = i < n_rows - 1;
        left[i] = left_step(i, n_rows, prev ? lcp(key[order[i - 1]], key[order[i]]) : 0, prev ? d[order[i - 1]] : 0);
        right[n - 1 - i] = right_step(i, n_rows, next ? lcp(key[order[i]], key[order[i + 1]]) : 0, next ? d[order[i + 1]] : 0);
    }
    for (int i = 1; i < n; i++) {
        left[i] = clamp_then(left[i - 1], left[i]);
        right[i] = clamp_then(right[i - 1], right[i]);
    }
    for (int i = 0; i < n; i++) {
        const int row = order[i];
        lkey[row] = kAbsent;
        if (i >= n_rows) continue;
        D[row] = final_depth(d[row], left[i], right[n - 1 - i]);
        lkey[row] = leaf_key(key[row], D[row]);
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lkey[a] < lkey[b]; });
    int n_leaves = 0;
    for (int j = 0; j < n; j++) {
        rows[j] = j < n_rows ? order[j] : 0;
        cell_start[j + 1] = 0;
        cell_width[j] = 0.0f;
        cell_level[j] = 0;
        for (int k = 0; k < 3; k++) {
            cell_center[3 * (size_t)j + k] = 0.0f;
            if (patch_center) patch_center[3 * (size_t)j + k] = 0.0f;
        }
        if (leaf_keys) leaf_keys[j] = 0;
    }
    for (int j = 0; j < n_rows; j++) {
        const int row = order[j];
        if (j > 0 && lkey[row] == lkey[order[j - 1]]) continue;
        const int l = n_leaves++;
        const float* p = center + 4 * (size_t)row;
        cell_start[l] = j;
        descend(r, p, D[row], cell_center + 3 * (size_t)l, cell_width[l]);
        cell_level[l] = D[row];
        if (patch_center)
            for (int k = 0; k < 3; k++) patch_center[3 * (size_t)l + k] = p[k];
        if (leaf_keys) leaf_keys[l] = lkey[row];
    }
    cell_start[n_leaves] = n_rows;
    float* fi = (float*)info;
    int32_t* ii = (int32_t*)info;
    fi[0] = r.c[0]; fi[1] = r.c[1]; fi[2] = r.c[2]; fi[3] = r.w; fi[4] = r.floor;
    ii[5] = n_rows; ii[6] = n_leaves;
    return 0;
}

// clamp_then(clamp_then(a, b), c) and clamp_then(a, clamp_then(b, c)) for (lo, hi) triples: out [2][2]
void st_clamp_assoc(const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out) {
    const Clamp A{a[0], a[1]}, B{b[0], b[1]}, Cc{c[0], c[1]};
    const Clamp x = clamp_then(clamp_then(A, B), Cc), y = clamp_then(A, clamp_then(B, Cc));
    out[0] = x.lo; out[1] = x.hi; out[2] = y.lo; out[3] = y.hi;
}

int st_depth_alone(float root_width, float width) { return depth_alone(root_width, width); }

}  // extern "C"
