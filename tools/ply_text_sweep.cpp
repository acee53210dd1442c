// ply_text_sweep -- the float-to-text conversion of hpmvs_amd/csrc/ply_text.hpp against this machine's snprintf("%.6g") over the
// bit patterns 0, stride, 2 stride, ... below 2^32 (stride 1: all of them), byte for byte and in length.  Host code only.
//   g++ -std=c++14 -O2 -fopenmp tools/ply_text_sweep.cpp -o ply_text_sweep && ./ply_text_sweep [stride] > profiles/ply_text_sweep.json
// prints one JSON line: the stride, the patterns compared, the mismatches and the first mismatching pattern; exit status 1 when
// there is a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hpmvs_amd/csrc/ply_text.hpp"

using namespace hpmvs::ply;

int main(int argc, char** argv) {
    const unsigned long long stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull;
    if (stride < 1 || stride > 0xFFFFFFFFull) { fprintf(stderr, "usage: ply_text_sweep [stride 1 .. 2^32 - 1]\n"); return 2; }
    const long long count = (long long)((0x100000000ull + stride - 1) / stride);
    long long bad = 0;
    unsigned long long first_bad = ~0ull;
#pragma omp parallel for schedule(static) reduction(+ : bad) reduction(min : first_bad)
    for (long long i = 0; i < count; i++) {
        const uint32_t bits = (uint32_t)((unsigned long long)i * stride);
        float f;
        memcpy(&f, &bits, 4);
        char want[32], got[16];
        const int wn = snprintf(want, sizeof(want), "%.6g", (double)f);
        const uint32_t rec = float_record(bits);
        const int gn = put_float(rec, got);
        if (gn != wn || gn != float_len(rec) || memcmp(want, got, (size_t)gn) != 0) {
            bad++;
            if (bits < first_bad) first_bad = bits;
        }
    }
    printf("{\"stride\": %llu, \"patterns\": %lld, \"mismatches\": %lld, \"first_mismatch\": ", stride, count, bad);
    if (bad) printf("\"0x%08llx\"}\n", first_bad); else printf("null}\n");
    return bad ? 1 : 0;
}
