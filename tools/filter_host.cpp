// Host restatement of CellProcessor::filter (reference src/hpmvs/CellProcessor.cpp:43-82) for tools/filter_level_scale.py: the cells
// of a level on `threads` OpenMP threads, cell by cell as the reference runs them (float arithmetic, no contraction: build with
// -ffp-contract=off).  Returns the wall time in seconds; keep[c] as hpmvs_filter_batch (-1 empty, -2 no winner).
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <omp.h>

extern "C" double filter_host(const float* center, const float* normal, const int32_t* cs, int n_cells, int threads, float* dist,
                              int32_t* keep) {
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 64) num_threads(threads)
    for (int c = 0; c < n_cells; c++) {
        const int s = cs[c], e = cs[c + 1], k = e - s;
        if (k < 2) {
            if (k == 1) dist[s] = 0.0f;
            keep[c] = k == 1 ? s : -1;
            continue;
        }
        float best = FLT_MAX;
        int idx = -2;
        for (int r = s; r < e; r++) {
            float n[3] = {normal[4 * r], normal[4 * r + 1], normal[4 * r + 2]};
            const float n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            if (n2 > 0.0f) { const float l = std::sqrt(n2); n[0] /= l; n[1] /= l; n[2] /= l; }
            float d = 0.0f;
            for (int j = s; j < e; j++) {
                if (j == r) continue;
                const float b0 = center[4 * j] - center[4 * r], b1 = center[4 * j + 1] - center[4 * r + 1], b2 = center[4 * j + 2] - center[4 * r + 2];
                d += (n[0] * b0 + n[1] * b1) + n[2] * b2;
            }
            d /= (float)(k - 1);
            dist[r] = d;
            if (d < best) { best = d; idx = r; }
        }
        keep[c] = idx;
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
