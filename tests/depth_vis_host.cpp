// Host restatement of the depth-map images: the product's empty-cell rule, minimum over the levels, normalise-and-index
// arithmetic and colormap (hpmvs_amd/csrc/depth_vis.hpp, the functions kernel_depth_vis.hip calls) compiled by g++ and run in
// plain loops.  tests/test_cpu_depth_vis.py pins it to CImg's normalize(0, 255) + map(jet_LUT256()) byte for byte
// (tests/golden/g9_depth_vis.npz); the GPU tests compare the kernels with the same images.
// Build: g++ -std=c++14 -O2 -ffp-contract=off -fPIC -shared depth_vis_host.cpp
#include <cstdint>
#include <vector>

#include "../hpmvs_amd/csrc/depth_vis.hpp"

using namespace hpmvs::dvis;

extern "C" {

void dv_colormap(uint8_t* lut) { make_colormap(lut); }

// cells: one map, column-major, element (y, x) at y + x * rows -> rgb [rows][cols][3]; range: m, M as used
void dv_level_image(const float* cells, int rows, int cols, uint8_t* rgb, float* range) {
    const size_t n = (size_t)rows * cols;
    if (!n) { range[0] = range[1] = 0.0f; return; }
    uint8_t lut[768];
    make_colormap(lut);
    std::vector<float> vals(n);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) vals[(size_t)y * cols + x] = cell_value(cells[(size_t)y + (size_t)x * rows]);
    float m = vals[0], M = vals[0];
    for (size_t i = 1; i < n; i++) { m = vals[i] < m ? vals[i] : m; M = vals[i] > M ? vals[i] : M; }
    for (size_t i = 0; i < n; i++) {
        const int k = lut_index(vals[i], m, M);
        for (int c = 0; c < 3; c++) rgb[3 * i + c] = lut[3 * k + c];
    }
    range[0] = m; range[1] = M;
}

// the combined map of n_levels column-major maps as ONE column-major map of level 0's shape (then dv_level_image)
void dv_combined(const float* const* d, const int32_t* rows, const int32_t* cols, int n_levels, float* out) {
    for (int x = 0; x < cols[0]; x++)
        for (int y = 0; y < rows[0]; y++) out[(size_t)y + (size_t)x * rows[0]] = combined_depth(d, rows, cols, n_levels, x, y);
}

}  // extern "C"
