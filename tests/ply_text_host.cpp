// Host restatement of the patch cloud's PLY file: the product's float-to-text conversion, integer writers, line and record
// builders and header (hpmvs_amd/csrc/ply_text.hpp, the functions kernel_ply.hip calls) compiled by g++ and run in plain loops.
// tests/test_cpu_ply_text.py pins it to this machine's C library (snprintf "%.6g") and to Python's formatting; the GPU tests
// compare the kernels with files built by Python.
// Build: g++ -std=c++14 -O2 -ffp-contract=off -fPIC -shared ply_text_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../hpmvs_amd/csrc/ply_text.hpp"

using namespace hpmvs::ply;

extern "C" {

// text [n][16] (NUL padded) and len [n] of the floats with these bit patterns; returns how often float_len disagrees with put_float
long pt_format(const uint32_t* bits, size_t n, char* text, int32_t* len) {
    long bad = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t rec = float_record(bits[i]);
        memset(text + 16 * i, 0, 16);
        len[i] = put_float(rec, text + 16 * i);
        if (len[i] != float_len(rec)) bad++;
    }
    return bad;
}

// The patterns first, first + stride, ... (count of them, modulo 2^32) against snprintf("%.6g"), byte for byte and in length:
// returns the mismatches, the first one's pattern in *first_bad.
long pt_check_snprintf(uint32_t first, uint32_t stride, uint64_t count, uint32_t* first_bad) {
    long bad = 0;
    uint32_t bits = first;
    for (uint64_t i = 0; i < count; i++, bits += stride) {
        float f;
        memcpy(&f, &bits, 4);
        char want[32], got[16];
        const int wn = snprintf(want, sizeof(want), "%.6g", (double)f);
        const uint32_t rec = float_record(bits);
        const int gn = put_float(rec, got);
        if (gn != wn || gn != float_len(rec) || memcmp(want, got, (size_t)gn) != 0) {
            if (!bad && first_bad) *first_bad = bits;
            bad++;
        }
    }
    return bad;
}

// the same for a list of patterns
long pt_check_list(const uint32_t* bits, size_t n, uint32_t* first_bad) {
    long bad = 0;
    for (size_t i = 0; i < n; i++) {
        uint32_t b = 0;
        if (pt_check_snprintf(bits[i], 0, 1, &b)) { if (!bad && first_bad) *first_bad = bits[i]; bad++; }
    }
    return bad;
}

void pt_colour_bytes(const uint32_t* bits, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; i++) out[i] = (uint8_t)colour_byte(bits[i]);
}

// The whole file for rows order[0 .. n_rows - 1] (order == NULL: rows 0 .. n_rows - 1) of the arrays center [n][4], normal [n][4],
// scale [n], color [n][3], n_images [n], images [n][max_images]; out == NULL: the length only.
size_t pt_file(const float* center, const float* normal, const float* scale, const float* color, const int32_t* n_images,
               const int32_t* images, int max_images, const int32_t* order, int n_rows, int flags, uint8_t* out) {
    const std::string h = header(n_rows, flags);
    size_t at = h.size();
    if (out) memcpy(out, h.data(), h.size());
    uint8_t line[kMaxVertexLine];
    for (int r = 0; r < n_rows; r++) {
        const size_t p = order ? (size_t)order[r] : (size_t)r;
        uint32_t v[kRowRecords];
        memcpy(v, center + 4 * p, 12);
        memcpy(v + 3, normal + 4 * p, 12);
        memcpy(v + 6, color + 3 * p, 12);
        memcpy(v + 9, scale + p, 4);
        int n;
        if (flags & kBinary) {
            n = put_vertex_record(v, v + 3, v + 6, v[9], flags, line);
            if (n != vertex_record_len(flags)) return 0;
        } else {
            uint32_t rec[kRowRecords];
            for (int k = 0; k < kRowRecords; k++) rec[k] = (k >= 6 && k < 9) ? colour_byte(v[k]) : float_record(v[k]);
            n = put_vertex_line(rec, 1, flags, line);
            if (n != vertex_line_len(rec, 1, flags)) return 0;
        }
        if (out) memcpy(out + at, line, (size_t)n);
        at += (size_t)n;
    }
    if (flags & kVisibility) {
        std::string text;
        for (int r = 0; r < n_rows; r++) {
            const size_t p = order ? (size_t)order[r] : (size_t)r;
            const int n = n_images[p];
            const int32_t* ids = images + p * (size_t)max_images;
            if (flags & kBinary) {
                text.resize(list_record_len(n));
                put_le32((uint32_t)n, &text[0]);
                for (int k = 0; k < n; k++) put_le32((uint32_t)ids[k], &text[4 + 4 * (size_t)k]);
            } else {
                text.resize(list_line_len(n, ids));
                if (put_list_line(n, ids, &text[0]) != text.size()) return 0;
            }
            if (out) memcpy(out + at, text.data(), text.size());
            at += text.size();
        }
    }
    return at;
}

}  // extern "C"
