// ply_text.hpp -- the bytes of the reference's DynOctTree::toExtPly (include/hpmvs/doctree.h:526-622), written once for the
// device kernels (kernel_ply.hip), the C ABI (capi.hip) and the host restatement the tests compile with g++
// (tests/ply_text_host.cpp, tools/ply_text_sweep.cpp).  Integer arithmetic throughout: no float operation, no log10, no pow, no
// 128-bit division.
//
// A float in text is what `ostream << float` writes with default flags, i.e. printf("%.6g", (double)f): the six leading decimal
// digits of the EXACT binary value, the seventh and everything behind it rounded half-even, fixed notation when the decimal
// exponent X after rounding satisfies -4 <= X < 6 and scientific otherwise, trailing zeros and a bare point dropped.
//
// Exactness: |v| = m * 2^e with m < 2^24.  For e >= 0 the value is the integer m << e (at most 128 bits); for e < 0 it is
// m * 5^-e / 10^-e, and m * 5^-e is an integer of at most 371 bits.  Either integer is held in twelve 32-bit limbs and turned
// into base-1e9 chunks by short division (a 64-bit dividend over a constant), so every decimal digit of the value exists
// before one is dropped: the first seven significant digits plus one sticky bit for the rest decide the rounding, and a carry out
// of 999999 moves the exponent.  Nothing is estimated, so nothing can be off by one.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define HPMVS_PLY_FN __host__ __device__ inline
#else
#define HPMVS_PLY_FN inline
#endif

namespace hpmvs {
namespace ply {

constexpr int kBinary = 1, kNormal = 2, kScale = 4, kVisibility = 8, kAllFlags = 15;  // HPMVS_PLY_*
constexpr int kMaxFloatText = 12;      // "-1.17549e-38", "-0.000123457"
constexpr int kRowRecords = 10;        // x y z nx ny nz r g b scale
// the longest vertex line: seven floats and three colours, each with its space, and the newline
constexpr int kMaxVertexLine = 7 * (kMaxFloatText + 1) + 3 * 4 + 1;
constexpr int kMaxVertexRecord = 31;   // binary: 3 floats, 3 floats, 3 bytes, 1 float

// ------------------------------------------------------------------------------------------------ the digit record
// bits 0-19: the six digits as an integer 100000 .. 999999 (0 for a zero and the specials); bits 20-26: the decimal exponent
// X + 64 (value = d.ddddd * 10^X); bit 27: the sign; bits 28-29: the class.
constexpr uint32_t kFinite = 0, kInf = 1, kNan = 2;
HPMVS_PLY_FN uint32_t make_record(uint32_t digits, int X, uint32_t sign, uint32_t cls) {
    return digits | ((uint32_t)(X + 64) << 20) | (sign << 27) | (cls << 28);
}
HPMVS_PLY_FN uint32_t rec_digits(uint32_t r) { return r & 0xFFFFFu; }
HPMVS_PLY_FN int rec_exp(uint32_t r) { return (int)((r >> 20) & 127u) - 64; }
HPMVS_PLY_FN uint32_t rec_sign(uint32_t r) { return (r >> 27) & 1u; }
HPMVS_PLY_FN uint32_t rec_class(uint32_t r) { return (r >> 28) & 3u; }

HPMVS_PLY_FN uint32_t pow10_u32(int k) {   // k = 0 .. 9
    switch (k) {
    case 0: return 1u;
    case 1: return 10u;
    case 2: return 100u;
    case 3: return 1000u;
    case 4: return 10000u;
    case 5: return 100000u;
    case 6: return 1000000u;
    case 7: return 10000000u;
    case 8: return 100000000u;
    default: return 1000000000u;
    }
}
HPMVS_PLY_FN uint32_t pow5_u32(int k) {   // k = 0 .. 13
    uint32_t p = 1u;
    for (int i = 0; i < k; i++) p *= 5u;
    return p;
}
HPMVS_PLY_FN int dec_digits(uint32_t v) {   // decimal digits of v, 1 for 0
    int d = 1;
    while (d < 10 && v >= pow10_u32(d)) d++;
    return d;
}

// the bit pattern of a float -> its record
HPMVS_PLY_FN uint32_t float_record(uint32_t bits) {
    const uint32_t sign = bits >> 31, be = (bits >> 23) & 255u, frac = bits & 0x7FFFFFu;
    if (be == 255u) return make_record(0, 0, sign, frac ? kNan : kInf);
    if (be == 0u && frac == 0u) return make_record(0, 0, sign, kFinite);
    const uint32_t m = be ? (frac | 0x800000u) : frac;
    const int e = (be ? (int)be : 1) - 150;   // |v| = m * 2^e
    constexpr int kLimbs = 12;
    uint32_t L[kLimbs];
    for (int i = 0; i < kLimbs; i++) L[i] = 0u;
    int n = 1, places = 0;   // limbs in use; decimal places behind the point
    if (e >= 0) {
        const int w = e >> 5, s = e & 31;
        L[w] = m << s;
        if (s) L[w + 1] = (uint32_t)(((uint64_t)m << s) >> 32);
        n = w + 2;
    } else {
        places = -e;
        L[0] = m;
        for (int k = places; k > 0; k -= 13) {
            const uint64_t f = pow5_u32(k < 13 ? k : 13);   // 5^13 < 2^31
            uint64_t carry = 0;
            for (int i = 0; i < n; i++) {
                const uint64_t t = (uint64_t)L[i] * f + carry;
                L[i] = (uint32_t)t;
                carry = t >> 32;
            }
            if (carry) L[n++] = (uint32_t)carry;   // (371 bits at most: n stays within kLimbs)
        }
    }
    while (n > 1 && L[n - 1] == 0u) n--;
    // base-1e9 chunks from the least significant up; only the two leading ones and whether the rest is zero are kept
    uint32_t hi = 0u, lo = 0u;
    bool has_lo = false, rest = false;
    int chunks = 0;
    while (n > 1 || L[0] != 0u) {
        uint64_t rem = 0;
        for (int i = n - 1; i >= 0; i--) {
            const uint64_t t = (rem << 32) | L[i];
            L[i] = (uint32_t)(t / 1000000000u);
            rem = t % 1000000000u;
        }
        while (n > 1 && L[n - 1] == 0u) n--;
        if (has_lo && lo != 0u) rest = true;
        if (chunks > 0) { lo = hi; has_lo = true; }
        hi = (uint32_t)rem;
        chunks++;
    }
    const int d = dec_digits(hi);
    int X = 9 * (chunks - 1) + d - 1 - places;
    // the first seven significant digits and the sticky bit behind them
    uint32_t S;
    bool sticky = rest;
    if (d >= 7) {
        const uint32_t p = pow10_u32(d - 7);
        S = hi / p;
        sticky = sticky || (hi % p) != 0u || lo != 0u;
    } else {
        const uint32_t p = pow10_u32(2 + d);   // of lo's nine digits the leading 7 - d are taken
        S = hi * pow10_u32(7 - d) + (has_lo ? lo / p : 0u);
        sticky = sticky || (has_lo && (lo % p) != 0u);
    }
    uint32_t q = S / 10u;
    const uint32_t r = S % 10u;
    if (r > 5u || (r == 5u && (sticky || (q & 1u)))) q++;
    if (q == 1000000u) { q = 100000u; X++; }
    return make_record(q, X, sign, kFinite);
}

HPMVS_PLY_FN int sig_digits(uint32_t q) {   // of the six digits, how many remain without the trailing zeros (q != 0)
    int n = 6;
    while (n > 1 && q % 10u == 0u) { q /= 10u; n--; }
    return n;
}

// the length of a record's text, 1 .. kMaxFloatText
HPMVS_PLY_FN int float_len(uint32_t rec) {
    const int sign = (int)rec_sign(rec);
    if (rec_class(rec) != kFinite) return sign + 3;
    const uint32_t q = rec_digits(rec);
    if (q == 0u) return sign + 1;
    const int X = rec_exp(rec), ns = sig_digits(q);
    if (X < -4 || X >= 6) return sign + (ns > 1 ? ns + 1 : 1) + 4;   // d[.ddddd]e+XX: a float's exponent has two digits
    if (X >= 0) return sign + (ns > X + 1 ? ns + 1 : X + 1);
    return sign + 1 - X + ns;   // 0. then -X - 1 zeros
}

// the text of a record at out; returns its length
template <typename Byte>
HPMVS_PLY_FN int put_float(uint32_t rec, Byte* out) {
    int at = 0;
    if (rec_sign(rec)) out[at++] = (Byte)'-';
    const uint32_t cls = rec_class(rec);
    if (cls == kInf) { out[at++] = (Byte)'i'; out[at++] = (Byte)'n'; out[at++] = (Byte)'f'; return at; }
    if (cls == kNan) { out[at++] = (Byte)'n'; out[at++] = (Byte)'a'; out[at++] = (Byte)'n'; return at; }
    const uint32_t q = rec_digits(rec);
    if (q == 0u) { out[at++] = (Byte)'0'; return at; }
    const int X = rec_exp(rec), ns = sig_digits(q);
    const bool sci = X < -4 || X >= 6;
    const int lead = (sci || X < 0) ? 1 : X + 1;   // digits in front of the point
    if (!sci && X < 0) {
        out[at++] = (Byte)'0';
        out[at++] = (Byte)'.';
        for (int k = 0; k < -X - 1; k++) out[at++] = (Byte)'0';
    }
    uint32_t rem = q, p = 100000u;
    const int shown = (!sci && X >= 0 && ns < lead) ? lead : ns;   // 123000 -> "123000": zeros in front of the point stay
    for (int k = 0; k < shown; k++) {
        if (k == lead && !(!sci && X < 0)) out[at++] = (Byte)'.';
        const uint32_t dgt = rem / p;
        rem -= dgt * p;
        p /= 10u;
        out[at++] = (Byte)('0' + dgt);
    }
    if (sci) {
        const int a = X < 0 ? -X : X;
        out[at++] = (Byte)'e';
        out[at++] = (Byte)(X < 0 ? '-' : '+');
        out[at++] = (Byte)('0' + a / 10);
        out[at++] = (Byte)('0' + a % 10);
    }
    return at;
}

// ------------------------------------------------------------------------------------------------ integers
HPMVS_PLY_FN int uint_len(uint32_t v) { return dec_digits(v); }
template <typename Byte>
HPMVS_PLY_FN int put_uint(uint32_t v, Byte* out) {
    const int n = dec_digits(v);
    for (int k = n - 1; k >= 0; k--) { out[k] = (Byte)('0' + v % 10u); v /= 10u; }
    return n;
}

// A colour channel: the float truncated towards zero, as (unsigned char) of a value in [0, 256) does; below 0 it is 0, from 256
// up it is 255, a NaN is 0 (the reference's conversion is undefined there).  From the bit pattern, without a float operation.
HPMVS_PLY_FN uint32_t colour_byte(uint32_t bits) {
    const uint32_t be = (bits >> 23) & 255u, frac = bits & 0x7FFFFFu;
    if (be == 255u && frac) return 0u;      // NaN
    if (bits >> 31) return 0u;              // negative, -0, -inf
    if (be < 127u) return 0u;               // below 1
    if (be >= 135u) return 255u;            // from 256 up, +inf
    return (frac | 0x800000u) >> (150u - be);   // 1 <= v < 256: 23 - (be - 127) fraction bits go
}

// ------------------------------------------------------------------------------------------------ lines and records
// rec[k * stride]: the row's records x y z nx ny nz r g b scale; the colours are held as their bytes 0 .. 255.
HPMVS_PLY_FN int vertex_line_len(const uint32_t* rec, size_t stride, int flags) {
    int n = 1;
    for (int k = 0; k < 3; k++) n += float_len(rec[k * stride]) + 1;
    if (flags & kNormal)
        for (int k = 3; k < 6; k++) n += float_len(rec[k * stride]) + 1;
    for (int k = 6; k < 9; k++) n += uint_len(rec[k * stride]) + 1;
    if (flags & kScale) n += float_len(rec[9 * stride]) + 1;
    return n;
}
template <typename Byte>
HPMVS_PLY_FN int put_vertex_line(const uint32_t* rec, size_t stride, int flags, Byte* out) {
    int at = 0;
    for (int k = 0; k < 3; k++) { at += put_float(rec[k * stride], out + at); out[at++] = (Byte)' '; }
    if (flags & kNormal)
        for (int k = 3; k < 6; k++) { at += put_float(rec[k * stride], out + at); out[at++] = (Byte)' '; }
    for (int k = 6; k < 9; k++) { at += put_uint(rec[k * stride], out + at); out[at++] = (Byte)' '; }
    if (flags & kScale) { at += put_float(rec[9 * stride], out + at); out[at++] = (Byte)' '; }
    out[at++] = (Byte)'\n';
    return at;
}
HPMVS_PLY_FN int vertex_record_len(int flags) { return 15 + ((flags & kNormal) ? 12 : 0) + ((flags & kScale) ? 4 : 0); }
template <typename Byte>
HPMVS_PLY_FN void put_le32(uint32_t v, Byte* out) {
    out[0] = (Byte)(v & 255u); out[1] = (Byte)((v >> 8) & 255u); out[2] = (Byte)((v >> 16) & 255u); out[3] = (Byte)(v >> 24);
}
// the binary vertex record from the bit patterns xyz[3], nrm[3], colour bits[3], scale
template <typename Byte>
HPMVS_PLY_FN int put_vertex_record(const uint32_t* xyz, const uint32_t* nrm, const uint32_t* col, uint32_t scale, int flags, Byte* out) {
    int at = 0;
    for (int k = 0; k < 3; k++) { put_le32(xyz[k], out + at); at += 4; }
    if (flags & kNormal)
        for (int k = 0; k < 3; k++) { put_le32(nrm[k], out + at); at += 4; }
    for (int k = 0; k < 3; k++) out[at++] = (Byte)colour_byte(col[k]);
    if (flags & kScale) { put_le32(scale, out + at); at += 4; }
    return at;
}
// the visibility line "n id id ... \n" (n as int, an id as uint32_t) and the binary list
HPMVS_PLY_FN size_t list_line_len(int n, const int32_t* ids) {
    size_t len = (size_t)uint_len((uint32_t)n) + 2;
    for (int k = 0; k < n; k++) len += (size_t)uint_len((uint32_t)ids[k]) + 1;
    return len;
}
template <typename Byte>
HPMVS_PLY_FN size_t put_list_line(int n, const int32_t* ids, Byte* out) {
    size_t at = (size_t)put_uint((uint32_t)n, out);
    out[at++] = (Byte)' ';
    for (int k = 0; k < n; k++) { at += (size_t)put_uint((uint32_t)ids[k], out + at); out[at++] = (Byte)' '; }
    out[at++] = (Byte)'\n';
    return at;
}
HPMVS_PLY_FN size_t list_record_len(int n) { return 4 + 4 * (size_t)n; }

// ------------------------------------------------------------------------------------------------ the header (host)
inline std::string header(int n_rows, int flags) {   // doctree.h:544-569, every std::endl a '\n'
    const std::string count = std::to_string(n_rows);
    std::string h = "ply\n";
    h += (flags & kBinary) ? "format binary_little_endian 1.0\n" : "format ascii 1.0\n";
    h += "element vertex " + count + "\n";
    h += "property float x\nproperty float y\nproperty float z\n";
    if (flags & kNormal) h += "property float nx\nproperty float ny\nproperty float nz\n";
    h += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    if (flags & kScale) h += "property float scalar_scale\n";
    if (flags & kVisibility) h += "element point_visibility " + count + "\nproperty list uint uint visible_cameras\n";
    h += "end_header\n";
    return h;
}

}  // namespace ply
}  // namespace hpmvs
