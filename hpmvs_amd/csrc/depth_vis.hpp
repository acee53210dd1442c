// depth_vis.hpp -- a depth map as a jet-coloured image (reference Scene::visualizeDepths, src/hpmvs/Scene.cpp:434-516, through
// CImg's normalize(0, 255), map() and jet_LUT256()), written once for the device kernels (kernel_depth_vis.hip), the C ABI
// (capi_image.hip) and the host restatement the tests compile with g++ (tests/depth_vis_host.cpp).  Float32 throughout, no
// contraction: the image equals the reference's byte for byte (tests/golden/g9_depth_vis.npz).
//
// The steps: a map cell (or, for the combined image, the minimum over the pyramid levels) becomes a VALUE, 0 when the cell is
// empty; m and M are the least and the largest value of the image; every value becomes a colormap index 0 .. 255 by the three
// cases of normalize(); the index picks an RGB entry of the 256-entry colormap.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HPMVS_DVIS_FN __host__ __device__ inline
#else
#define HPMVS_DVIS_FN inline
#endif

namespace hpmvs {
namespace dvis {

constexpr float kMaxDepth = 1000.0f;  // Scene::MAX_DEPTH (Scene.cpp:33): an empty cell
constexpr float kFloatMax = 3.402823466e+38f;

// ------------------------------------------------------------------------------------------------ the empty-cell rule
// A cell that is no finite number holds nothing (the reference's result for one is undefined: its min / max depend on where a
// NaN sits, and the NaN is then cast to an integer).  Plain float comparisons: NaN fails both, an infinity the second.
HPMVS_DVIS_FN bool is_finite(float v) { return v >= -kFloatMax && v <= kFloatMax; }
// the cell as the minimum over the levels sees it: what holds nothing is MAX_DEPTH
HPMVS_DVIS_FN float cell_depth(float v) { return is_finite(v) ? v : kMaxDepth; }
// the image's value: `if (v == MAX_DEPTH) v = 0` (Scene.cpp:477-478, 498-499).  Negative finite cells are ordinary values.
HPMVS_DVIS_FN float cell_value(float v) { return (!is_finite(v) || v == kMaxDepth) ? 0.0f : v; }

// Scene::getFullDepth(view, 2 x, 2 y) (Scene.cpp:406-432; full_depth() of kernel_depth.hip is the same walk for the gates): the
// minimum over the levels of the cell at (x >> l, y >> l), from MAX_DEPTH, returning at the first level where that cell is
// outside the map (odd level sizes: a 35-column level 0 over a 17-column level 1 leaves at x = 34).  d[l]: level l's map,
// column-major, element (y, x) at y + x * rows[l].
HPMVS_DVIS_FN float combined_depth(const float* const* d, const int32_t* rows, const int32_t* cols, int n_levels, int x, int y) {
    float depth = kMaxDepth;
    for (int l = 0; l < n_levels; l++) {
        if (x >= cols[l] || y >= rows[l]) return depth;
        const float v = cell_depth(d[l][(size_t)y + (size_t)x * (size_t)rows[l]]);
        depth = v < depth ? v : depth;  // std::min(depth, v)
        x /= 2; y /= 2;
    }
    return depth;
}

// ------------------------------------------------------------------------------------------------ normalise and index
// CImg<float>::normalize(0, 255) followed by map()'s truncation, for one value v of an image whose values span m .. M:
//   m == M                 every pixel becomes 0 (an empty map, and a map whose cells all hold one depth)
//   m == 0 and M == 255    the image is left as it is
//   otherwise              (v - m) / (M - m) * 255 + 0, every operation a float32 one, the division IEEE's
// The result lies in 0 .. 255: v - m <= M - m, both rounded the same way, so the quotient is at most 1.
HPMVS_DVIS_FN int lut_index(float v, float m, float M) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (m == M) return 0;
    if (m == 0.0f && M == 255.0f) return (int)v;
    const float num = v - m, den = M - m;
    const float q = num / den;
    return (int)(q * 255.0f + 0.0f);
}

// ------------------------------------------------------------------------------------------------ the colormap
// CImg's "jet": per channel four control values, R 0 0 255 255, G 0 255 255 0, B 255 255 0 0, stretched to 256 entries by
// linear interpolation.  Entry i lies at t_i control intervals from the first value, where t_0 = 0 and t_(i+1) = t_i + s in
// float32 with s = (4 - 1.0f) / (256 - 1): the position is ACCUMULATED, rounding at every step, not computed as i * s.  With
// k = trunc(t_i) and a = t_i - k the entry is trunc((1 - a) * c[k] + a * c[k + 1]) in float32, c[k + 1] = c[k] behind the last
// control value.  That is not the textbook jet: entry 31 is 0 93 254, entry 127 is 126 255 128.
// lut: entry i at lut[3 i .. 3 i + 2].  Host only (the kernels read the table the host made).
inline void make_colormap(uint8_t lut[768]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    static const float ctl[3][4] = {{0.0f, 0.0f, 255.0f, 255.0f}, {0.0f, 255.0f, 255.0f, 0.0f}, {255.0f, 255.0f, 0.0f, 0.0f}};
    const float step = (4 - 1.0f) / (256 - 1);
    float t = 0.0f;
    for (int i = 0; i < 256; i++) {
        const unsigned k = (unsigned)t;
        const float a = t - (float)k;
        for (int c = 0; c < 3; c++) {
            const float v1 = ctl[c][k < 3 ? k : 3], v2 = k < 3 ? ctl[c][k + 1] : v1;
            const float lo = (1.0f - a) * v1, hi = a * v2;
            lut[3 * i + c] = (uint8_t)(lo + hi);
        }
        t += step;
    }
}

}  // namespace dvis
}  // namespace hpmvs
