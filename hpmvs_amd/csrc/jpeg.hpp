// jpeg.hpp -- baseline JPEG decoding of a view's level 0 (reference Image::load through CImg and libjpeg,
// src/hpmvs/Image.cpp:46, thirdLibs/cimg/CImg.h:36920-36934, library defaults: JDCT_ISLOW, fancy upsampling, the integer
// YCbCr conversion), written once for the device kernels (kernel_jpeg.hip), the C ABI (capi_image.hip) and the host
// restatement the tests compile with g++ (tests/jpeg_host.cpp).
//
// The split: the host parses the markers and either decodes the bit-serial entropy data into dense int16 coefficients
// itself (decode_scan, plain C++) or hands the scan to the device, which decodes it in parallel subsequences with
// decode_subseq (last part of this file; kernel_jpeg_entropy.hip); everything after the coefficients --
// dequantisation, the 8x8 integer IDCT, chroma interpolation, colour conversion -- is the arithmetic of the first half,
// which the kernels run per block and per pixel and the host restatement runs in loops.  All products and sums of the
// IDCT are formed on uint32_t and converted back, so that coefficients no encoder produces wrap identically on both
// sides instead of overflowing a signed int on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define HPMVS_JPG_FN __host__ __device__ inline
#else
#define HPMVS_JPG_FN inline
#endif

namespace hpmvs {
namespace jpg {

// ------------------------------------------------------------------------------------------------ shared arithmetic
// arithmetic right shift of a value kept in uint32_t
HPMVS_JPG_FN int32_t asr(uint32_t v, int s) { return (int32_t)v >> s; }

// One 1-D pass of libjpeg's jidctint (constants FIX(x) at 13 bits), rounded with (x + 2^(shift-1)) >> shift.
// Pass 1 runs down the columns of the dequantised block with shift 11, pass 2 along the rows of its result with shift 18.
HPMVS_JPG_FN void idct_1d(const int32_t* d, int32_t* o, int shift) {
    typedef uint32_t u;
    const u d0 = (u)d[0], d1 = (u)d[1], d2 = (u)d[2], d3 = (u)d[3], d4 = (u)d[4], d5 = (u)d[5], d6 = (u)d[6], d7 = (u)d[7];
    u z1 = (d2 + d6) * 4433u;
    const u t2 = z1 - d6 * 15137u;
    const u t3 = z1 + d2 * 6270u;
    const u t0 = (d0 + d4) << 13, t1 = (d0 - d4) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u a0 = d7, a1 = d5, a2 = d3, a3 = d1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5;
    z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const u r = 1u << (shift - 1);
    o[0] = asr(t10 + a3 + r, shift); o[7] = asr(t10 - a3 + r, shift);
    o[1] = asr(t11 + a2 + r, shift); o[6] = asr(t11 - a2 + r, shift);
    o[2] = asr(t12 + a1 + r, shift); o[5] = asr(t12 - a1 + r, shift);
    o[3] = asr(t13 + a0 + r, shift); o[4] = asr(t13 - a0 + r, shift);
}
constexpr int kPass1Shift = 11, kPass2Shift = 18;

// coefficient (libjpeg's JCOEF, a short) times its quantiser step
HPMVS_JPG_FN int32_t dequant(int16_t c, uint16_t q) { return (int32_t)((uint32_t)(int32_t)c * (uint32_t)q); }

// libjpeg's range-limit table behind the IDCT, indexed with the centred value & 1023: a clamp of v + 128 to 0..255 for
// -384 <= v < 640, and the table's wrap-around for anything a legal file cannot reach
HPMVS_JPG_FN uint8_t range_limit(int32_t v) {
    const uint32_t t = (uint32_t)v & 1023u;
    return (uint8_t)(t < 128u ? t + 128u : t < 512u ? 255u : t < 896u ? 0u : t - 896u);
}

HPMVS_JPG_FN uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// libjpeg's YCbCr -> RGB tables (16-bit fixed point, arithmetic shifts)
HPMVS_JPG_FN void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128;
    cr -= 128;
    rgb[0] = clamp255(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp255(y + ((116130 * cb + 32768) >> 16));
}

// Sample planes of a decoded frame, one per component, in one buffer: plane c starts at off[c], its rows are stride[c]
// bytes apart (blocks_x * 8, the block padding included).  Chroma planes hold dw x dh samples that count; the
// upsamplers replicate the first and last of THOSE rows and columns, never the padding.
struct Planes {
    int32_t W, H, ncomp;
    int32_t hs, vs;  // luma sampling factors = chroma subsampling (1x1, 2x1, 2x2); 1x1 for grayscale
    int32_t dw, dh;  // chroma plane size that counts
    uint32_t off[3];
    int32_t stride[3];
};

HPMVS_JPG_FN int imin(int a, int b) { return a < b ? a : b; }
HPMVS_JPG_FN int imax(int a, int b) { return a > b ? a : b; }

// Chroma of the four output pixels x0 .. x0+3 (x0 a multiple of 4) of row y: direct for 1x1, libjpeg's fancy h2v1 /
// h2v2 interpolation otherwise.  h2v1: out[2k] = (3 in[k] + in[k-1] + 1) >> 2, out[2k+1] = (3 in[k] + in[k+1] + 2) >> 2;
// h2v2: s[k] = 3 near[k] + far[k] (far = the row above for even y, below for odd y, clamped to the plane),
// out[2k] = (3 s[k] + s[k-1] + 8) >> 4, out[2k+1] = (3 s[k] + s[k+1] + 7) >> 4.  Clamping k-1 / k+1 to the plane gives
// libjpeg's edge columns (out[0] = in[0], out[last] = in[dw-1]).
HPMVS_JPG_FN void chroma4(const uint8_t* plane, int stride, const Planes& P, int x0, int y, int* c) {
    if (P.hs == 1) {
        const uint8_t* row = plane + (size_t)y * stride;
        for (int j = 0; j < 4; j++) c[j] = row[imin(x0 + j, P.W - 1)];
        return;
    }
    const int last = P.dw - 1;
    const int k0 = imin(x0 >> 1, last), km = imax(k0 - 1, 0), k1 = imin(k0 + 1, last), k2 = imin(k0 + 2, last);
    int sm, s0, s1, s2, even, odd, shift;
    if (P.vs == 1) {
        const uint8_t* row = plane + (size_t)y * stride;
        sm = row[km]; s0 = row[k0]; s1 = row[k1]; s2 = row[k2];
        even = 1; odd = 2; shift = 2;
    } else {
        const int i = y >> 1;
        const int f = (y & 1) ? imin(i + 1, P.dh - 1) : imax(i - 1, 0);
        const uint8_t* near = plane + (size_t)i * stride;
        const uint8_t* far = plane + (size_t)f * stride;
        sm = 3 * near[km] + far[km]; s0 = 3 * near[k0] + far[k0];
        s1 = 3 * near[k1] + far[k1]; s2 = 3 * near[k2] + far[k2];
        even = 8; odd = 7; shift = 4;
    }
    c[0] = (3 * s0 + sm + even) >> shift;
    c[1] = (3 * s0 + s1 + odd) >> shift;
    c[2] = (3 * s1 + s0 + even) >> shift;
    c[3] = (3 * s1 + s2 + odd) >> shift;
}

// interleaved RGB of the output pixels x0 .. x0+3 of row y (x0 a multiple of 4, x0 < W, y < H); pixels at x >= W are
// computed from clamped samples and must not be stored
HPMVS_JPG_FN void convert_quad(const uint8_t* planes, const Planes& P, int x0, int y, uint8_t* out) {
    const uint8_t* yrow = planes + P.off[0] + (size_t)y * P.stride[0] + x0;  // the padded row holds x0 .. x0+3
    if (P.ncomp == 1) {
        for (int j = 0; j < 4; j++) out[3 * j] = out[3 * j + 1] = out[3 * j + 2] = yrow[j];
        return;
    }
    int cb[4], cr[4];
    chroma4(planes + P.off[1], P.stride[1], P, x0, y, cb);
    chroma4(planes + P.off[2], P.stride[2], P, x0, y, cr);
    for (int j = 0; j < 4; j++) ycc_to_rgb(yrow[j], cb[j], cr[j], out + 3 * j);
}

// ------------------------------------------------------------------------------------------------ host: parser and entropy decoder
// (plain C++, no HIP: host functions only)
constexpr int kOk = 0, kErrArg = -2, kErrUnsupported = -5;  // HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED

struct Component {
    int id, h, v, tq, td, ta;
    int bx, by;   // blocks per row / column, padded to whole MCUs
    size_t off;   // first coefficient of the component in Frame::coef
};

struct Frame {
    int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1;
    int mcus_x = 0, mcus_y = 0, restart = 0;
    Component c[3];
    uint16_t q[3][64];          // per component, natural order
    size_t n_blocks = 0;        // of all components
    std::vector<int16_t> coef;  // per component [by][bx][64], natural order
};

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Huffman table: 9 bits of look-ahead resolve the common codes in one step, the canonical min / max codes the rest
struct Huff {
    bool defined = false;
    uint16_t lut[512];  // (length << 8) | symbol, 0 = longer than 9 bits or no code
    int32_t mincode[17], maxcode[17], valptr[17];
    uint8_t vals[256];
};

inline bool huff_build(Huff& h, const uint8_t* counts16, const uint8_t* vals, int nvals) {
    memset(h.lut, 0, sizeof(h.lut));
    memcpy(h.vals, vals, (size_t)nvals);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        h.valptr[l] = k;
        h.mincode[l] = code;
        for (int i = 0; i < counts16[l - 1]; i++, code++, k++) {
            if (code >= (1 << l)) return false;  // the counts describe no prefix code
            if (l <= 9)
                for (int f = 0; f < (1 << (9 - l)); f++) h.lut[(code << (9 - l)) + f] = (uint16_t)((l << 8) | vals[k]);
        }
        h.maxcode[l] = counts16[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.defined = true;
    return true;
}

// Entropy-coded bytes [pos, end): FF 00 is a literal FF, FF FF.. is fill, any other FF xx is a marker, where the reader
// stops.  Bits past the stop read as 0 but cannot be consumed, so a short segment is an error, never an over-read.
struct BitReader {
    const uint8_t* d;
    size_t pos, end;
    uint64_t buf = 0;  // left aligned
    int cnt = 0;       // valid bits in buf
    bool stop = false;
    void fill() {
        while (cnt <= 56 && !stop) {
            if (pos >= end) { stop = true; break; }
            uint8_t b = d[pos];
            if (b == 0xFF) {
                size_t q = pos + 1;
                while (q < end && d[q] == 0xFF) q++;
                if (q >= end || d[q] != 0) { stop = true; break; }
                pos = q + 1;
            } else {
                pos++;
            }
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    uint32_t peek(int n) {  // 1 <= n <= 16
        if (cnt < n) fill();
        return (uint32_t)(buf >> (64 - n));
    }
    bool consume(int n) {
        if (n > cnt) return false;
        buf <<= n;
        cnt -= n;
        return true;
    }
    // -> the expected RSTn, realigned to the byte behind it
    bool restart(int n) {
        buf = 0; cnt = 0; stop = false;
        if (pos >= end || d[pos] != 0xFF) return false;
        size_t q = pos + 1;
        while (q < end && d[q] == 0xFF) q++;
        if (q >= end || d[q] != 0xD0 + (n & 7)) return false;
        pos = q + 1;
        return true;
    }
};

inline int huff_decode(BitReader& br, const Huff& h) {
    const uint32_t e = h.lut[br.peek(9)];
    if (e >> 8) return br.consume((int)(e >> 8)) ? (int)(e & 255) : -1;
    for (int l = 10; l <= 16; l++) {
        const int32_t code = (int32_t)br.peek(l);
        if (h.maxcode[l] >= 0 && code >= h.mincode[l] && code <= h.maxcode[l])
            return br.consume(l) ? h.vals[h.valptr[l] + code - h.mincode[l]] : -1;
    }
    return -1;
}

// n extra bits -> the signed value (extend(v, n) of the standard); false: the data ended
inline bool receive_extend(BitReader& br, int n, int32_t* out) {
    if (n == 0) { *out = 0; return true; }
    const int32_t v = (int32_t)br.peek(n);
    if (!br.consume(n)) return false;
    *out = v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
    return true;
}

inline int fail(std::string* err, int code, const char* msg) {
    if (err) *err = std::string("jpeg: ") + msg;
    return code;
}

// The header parse of decode_file: everything in front of the entropy-coded bytes.  Fills fr (all but coef) and
// huff[8] ([class * 4 + id]) and gives the scan's first byte.  -> kOk, kErrArg (malformed, truncated) or kErrUnsupported
// (a legal file outside what is decoded here), with the reason in *err.
inline int parse_headers(const uint8_t* b, size_t n, Frame& fr, Huff* huff, size_t* scan_start, std::string* err) {
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return fail(err, kErrArg, "not a JPEG file (no SOI)");
    uint16_t qt[4][64];
    bool qt_set[4] = {false, false, false, false};
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    size_t i = 2;
    for (;;) {
        if (i >= n || b[i] != 0xFF) return fail(err, kErrArg, "marker expected");
        while (i < n && b[i] == 0xFF) i++;
        if (i >= n) return fail(err, kErrArg, "file ends inside the headers");
        const int m = b[i++];
        if (m == 0x01 || m == 0x00) return fail(err, kErrArg, "stray byte where a marker is expected");
        if (m >= 0xD0 && m <= 0xD7) return fail(err, kErrArg, "restart marker outside a scan");
        if (m == 0xD8) return fail(err, kErrArg, "second SOI");
        if (m == 0xD9) return fail(err, kErrArg, "EOI before any scan");
        if (i + 2 > n) return fail(err, kErrArg, "file ends inside the headers");
        const size_t L = ((size_t)b[i] << 8) | b[i + 1];
        if (L < 2 || i + L > n) return fail(err, kErrArg, "marker segment runs past the end of the file");
        const uint8_t* s = b + i + 2;
        const size_t sl = L - 2;
        i += L;
        if (m == 0xE0) {
            if (sl >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDB) {
            size_t k = 0;
            while (k < sl) {
                const int pq = s[k] >> 4, tq = s[k] & 15;
                if (pq == 1) return fail(err, kErrUnsupported, "16-bit quantisation table");
                if (pq > 1 || tq > 3) return fail(err, kErrArg, "bad quantisation table header");
                if (k + 65 > sl) return fail(err, kErrArg, "quantisation table runs past its segment");
                for (int z = 0; z < 64; z++) qt[tq][kZigzag[z]] = s[k + 1 + z];
                qt_set[tq] = true;
                k += 65;
            }
        } else if (m == 0xC4) {
            size_t k = 0;
            while (k < sl) {
                const int tc = s[k] >> 4, th = s[k] & 15;
                if (tc > 1 || th > 3) return fail(err, kErrArg, "bad Huffman table header");
                if (k + 17 > sl) return fail(err, kErrArg, "Huffman table runs past its segment");
                int nv = 0;
                for (int l = 0; l < 16; l++) nv += s[k + 1 + l];
                if (nv > 256 || k + 17 + (size_t)nv > sl) return fail(err, kErrArg, "Huffman table runs past its segment");
                if (tc == 0)
                    for (int v = 0; v < nv; v++)
                        if (s[k + 17 + v] > 15) return fail(err, kErrArg, "DC Huffman symbol above 15");
                if (!huff_build(huff[tc * 4 + th], s + k + 1, s + k + 17, nv)) return fail(err, kErrArg, "Huffman counts describe no prefix code");
                k += 17 + (size_t)nv;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return fail(err, kErrArg, "bad DRI length");
            fr.restart = (s[0] << 8) | s[1];
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return fail(err, kErrArg, "second frame header");
            if (sl < 6) return fail(err, kErrArg, "frame header too short");
            if (s[0] == 12) return fail(err, kErrUnsupported, "12-bit sample precision");
            if (s[0] != 8) return fail(err, kErrArg, "bad sample precision");
            fr.H = (s[1] << 8) | s[2];
            fr.W = (s[3] << 8) | s[4];
            fr.ncomp = s[5];
            if (fr.H == 0 || fr.W == 0) return fail(err, kErrArg, "frame header with zero width or height (DNL is not supported)");
            if (fr.ncomp == 0) return fail(err, kErrArg, "frame header without components");
            if (sl != 6 + 3 * (size_t)fr.ncomp) return fail(err, kErrArg, "bad frame header length");
            if (fr.ncomp == 4) return fail(err, kErrUnsupported, "four components (CMYK / YCCK)");
            if (fr.ncomp != 1 && fr.ncomp != 3) return fail(err, kErrUnsupported, "neither one nor three components");
            if (fr.W < 8 || fr.H < 8) return fail(err, kErrUnsupported, "image smaller than 8 pixels on a side");
            for (int c = 0; c < fr.ncomp; c++) {
                Component& C = fr.c[c];
                C.id = s[6 + 3 * c]; C.h = s[7 + 3 * c] >> 4; C.v = s[7 + 3 * c] & 15; C.tq = s[8 + 3 * c];
                if (C.h < 1 || C.h > 4 || C.v < 1 || C.v > 4 || C.tq > 3) return fail(err, kErrArg, "bad component in the frame header");
            }
            if (fr.ncomp == 1) {
                fr.c[0].h = fr.c[0].v = 1;  // a single component is never interleaved: its factors do not matter
            } else {
                const int h = fr.c[0].h, v = fr.c[0].v;
                const bool luma_ok = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma_ok || fr.c[1].h != 1 || fr.c[1].v != 1 || fr.c[2].h != 1 || fr.c[2].v != 1)
                    return fail(err, kErrUnsupported, "sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2)");
            }
            have_sof = true;
        } else if (m == 0xC2) {
            return fail(err, kErrUnsupported, "progressive JPEG (SOF2)");
        } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
            return fail(err, kErrUnsupported, m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF ? "lossless JPEG" :
                                              m >= 0xC9 ? "arithmetic-coded JPEG" : "hierarchical JPEG");
        } else if (m == 0xDA) {
            if (!have_sof) return fail(err, kErrArg, "scan before the frame header");
            if (sl < 1) return fail(err, kErrArg, "scan header too short");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return fail(err, kErrArg, "bad scan header length");
            if (ns != fr.ncomp) return fail(err, ns < fr.ncomp ? kErrUnsupported : kErrArg,
                                            ns < fr.ncomp ? "more than one scan (components not interleaved)" : "scan with more components than the frame");
            for (int c = 0; c < ns; c++) {
                Component& C = fr.c[c];
                if (s[1 + 2 * c] != C.id) {
                    for (int o = 0; o < ns; o++)
                        if (s[1 + 2 * c] == fr.c[o].id) return fail(err, kErrUnsupported, "scan components in another order than the frame's");
                    return fail(err, kErrArg, "scan names a component the frame does not have");
                }
                C.td = s[2 + 2 * c] >> 4; C.ta = s[2 + 2 * c] & 15;
                if (C.td > 3 || C.ta > 3 || !huff[C.td].defined || !huff[4 + C.ta].defined)
                    return fail(err, kErrArg, "scan uses a Huffman table that was not defined");
                if (!qt_set[C.tq]) return fail(err, kErrArg, "component uses a quantisation table that was not defined");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(err, kErrArg, "bad spectral selection for a sequential scan");
            break;
        }
        // APPn, COM and anything else with a length: skipped
    }
    // what libjpeg would take for RGB-coded data: JFIF wins, then the Adobe transform flag, then the component ids
    if (fr.ncomp == 3 && !jfif) {
        if (adobe ? adobe_transform == 0 : (fr.c[0].id == 'R' && fr.c[1].id == 'G' && fr.c[2].id == 'B'))
            return fail(err, kErrUnsupported, "RGB-coded components (no YCbCr transform)");
    }
    fr.hmax = fr.c[0].h;
    fr.vmax = fr.c[0].v;
    fr.mcus_x = (fr.W + 8 * fr.hmax - 1) / (8 * fr.hmax);
    fr.mcus_y = (fr.H + 8 * fr.vmax - 1) / (8 * fr.vmax);
    fr.n_blocks = 0;
    for (int c = 0; c < fr.ncomp; c++) {
        Component& C = fr.c[c];
        C.bx = fr.mcus_x * C.h;
        C.by = fr.mcus_y * C.v;
        C.off = fr.n_blocks * 64;
        fr.n_blocks += (size_t)C.bx * C.by;
        memcpy(fr.q[c], qt[C.tq], sizeof(qt[0]));
    }
    // plane offsets are 32-bit: frames of 4 Gi samples and more (65535 x 43690 in 4:2:0) are left out
    if (fr.n_blocks >= ((size_t)1 << 26) - 16) return fail(err, kErrUnsupported, "frame of 4 Gi samples or more");
    // a block takes two bits at the very least (a DC code and an end-of-block code): a header that promises more blocks
    // than the rest of the file can hold is refused before any buffer is sized by it
    if (fr.n_blocks > (n - i) * 4) return fail(err, kErrArg, "truncated: the entropy data cannot hold the frame's blocks");
    *scan_start = i;
    return kOk;
}

// The scan walk of decode_file over the entropy-coded bytes from scan_start on, with the frame and tables of
// parse_headers.  keep_coef: fill fr.coef; otherwise the data is walked and checked all the same.
inline int decode_scan(const uint8_t* b, size_t n, size_t scan_start, Frame& fr, const Huff* huff, bool keep_coef, std::string* err) {
    if (keep_coef) fr.coef.assign(fr.n_blocks * 64, 0);
    BitReader br{b, scan_start, n};
    int32_t pred[3] = {0, 0, 0};
    size_t mcu = 0;
    int rst = 0;
    for (int my = 0; my < fr.mcus_y; my++)
        for (int mx = 0; mx < fr.mcus_x; mx++, mcu++) {
            if (fr.restart && mcu && mcu % (size_t)fr.restart == 0) {
                if (!br.restart(rst++)) return fail(err, kErrArg, "restart marker missing or out of sequence");
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < fr.ncomp; c++) {
                const Component& C = fr.c[c];
                const Huff &dc = huff[C.td], &ac = huff[4 + C.ta];
                for (int by = 0; by < C.v; by++)
                    for (int bx = 0; bx < C.h; bx++) {
                        int16_t* blk = keep_coef ? &fr.coef[C.off + ((size_t)(my * C.v + by) * C.bx + (mx * C.h + bx)) * 64] : nullptr;
                        const int t = huff_decode(br, dc);
                        int32_t diff;
                        if (t < 0 || !receive_extend(br, t, &diff)) return fail(err, kErrArg, "truncated or corrupt entropy data");
                        pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)diff);
                        if (blk) blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = huff_decode(br, ac);
                            if (rs < 0) return fail(err, kErrArg, "truncated or corrupt entropy data");
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz == 0) {
                                if (r != 15) break;
                                k += 16;
                                continue;
                            }
                            k += r;
                            int32_t v;
                            if (k > 63) return fail(err, kErrArg, "corrupt entropy data: coefficient index past 63");
                            if (!receive_extend(br, sz, &v)) return fail(err, kErrArg, "truncated or corrupt entropy data");
                            if (blk) blk[kZigzag[k]] = (int16_t)v;
                            k++;
                        }
                    }
            }
        }
    // behind the scan: EOI.  Another scan means the first one did not hold the whole image.
    for (size_t p = br.pos; p + 1 < n; p++) {
        if (b[p] != 0xFF) continue;
        if (b[p + 1] == 0xD9) return kOk;
        if (b[p + 1] == 0xDA) return fail(err, kErrUnsupported, "more than one scan");
    }
    return fail(err, kErrArg, "truncated: no EOI behind the scan");
}

// Parses the file and decodes its one scan.  keep_coef: fill fr.coef; otherwise the entropy data is walked and checked
// all the same, without the coefficient buffer (hpmvs_jpeg_info).  -> kOk, kErrArg or kErrUnsupported, reason in *err.
inline int decode_file(const uint8_t* b, size_t n, Frame& fr, bool keep_coef, std::string* err) {
    std::vector<Huff> huff(8);
    size_t scan_start = 0;
    const int rc = parse_headers(b, n, fr, huff.data(), &scan_start, err);
    return rc != kOk ? rc : decode_scan(b, n, scan_start, fr, huff.data(), keep_coef, err);
}

// plane layout of a frame: offsets 256-byte aligned; -> bytes of the buffer
inline size_t make_planes(const Frame& fr, Planes* P) {
    P->W = fr.W; P->H = fr.H; P->ncomp = fr.ncomp;
    P->hs = fr.hmax; P->vs = fr.vmax;
    P->dw = (fr.W + fr.hmax - 1) / fr.hmax;
    P->dh = (fr.H + fr.vmax - 1) / fr.vmax;
    size_t total = 0;
    for (int c = 0; c < 3; c++) {
        P->off[c] = 0; P->stride[c] = 0;
        if (c >= fr.ncomp) continue;
        P->off[c] = (uint32_t)total;
        P->stride[c] = fr.c[c].bx * 8;
        total += ((size_t)fr.c[c].bx * fr.c[c].by * 64 + 255) & ~(size_t)255;
    }
    return total;
}

// ------------------------------------------------------------------------------------------------ parallel entropy decoding
// The scan's Huffman data decoded in parallel (kernel_jpeg_entropy.hip; restated in loops by tests/jpeg_entropy_host.cpp):
// the host removes the byte stuffing and cuts the scan at its restart markers into segments (prescan), every segment is
// cut into subsequences of S bits, and every subsequence is decoded by decode_subseq from an entry state -- first from a
// guess, then from its predecessor's exit until no exit changes (Huffman codes resynchronise after a wrong start).  A
// chain that a check accepts is the sequential decode of decode_scan, symbol for symbol.
constexpr int kSubseqBits = 512;      // the shipped subsequence size
constexpr int kSubsPerGroup = 64;     // subsequences that synchronise inside one workgroup (one wavefront)
// synchronisation rounds before the decode is left to the host: four times what the slowest fixture file needs at the
// shipped size (185); at another size (the test hook) as many rounds more as it has subsequences more
constexpr int kSyncRoundCap = 740;
HPMVS_JPG_FN int sync_round_cap(uint32_t subseq_bits) { return (int)((uint64_t)kSyncRoundCap * kSubseqBits / subseq_bits); }
constexpr uint32_t kStateErr = 1u << 31;

struct Segment {
    uint32_t first_byte;  // in the unstuffed bytes
    uint32_t bits;
    uint32_t first_mcu, n_mcus;
    uint32_t first_sub, n_subs;  // filled by plan_subsequences
};

// where a decoder stands: p bits into the segment, in block blk of the MCU (bk >> 8), at coefficient k (bk & 63; 0: the DC
// code comes next).  kStateErr in an exit's bk: the decode that gave it met an invalid code or k > 63.
struct SubState {
    uint32_t p, bk;
};
HPMVS_JPG_FN bool same_state(SubState a, SubState b) { return a.p == b.p && a.bk == b.bk; }
// the entry a subsequence takes from its predecessor's exit
HPMVS_JPG_FN SubState handed_on(SubState exit) {
    exit.bk &= ~kStateErr;
    return exit;
}

// what a subsequence adds to its segment: blocks completed and, per component, the sum of its DC differences (mod 2^32)
struct SubCount {
    uint32_t nblk, dc[3];
};

struct ScanInfo {
    int32_t ncomp, bpm;  // blocks per MCU
    int32_t mcus_x, n_mcus;
    int32_t h[3], v[3], bx[3];
    uint32_t off[3];  // first coefficient of the component
    uint8_t blk_comp[8], blk_dx[8], blk_dy[8];
};

// 32 bits of the segment from bit p on; bits past the segment's end read as 0.  d: the segment's first byte, with at least
// 8 readable bytes behind its last
HPMVS_JPG_FN uint32_t peek32(const uint8_t* d, uint32_t bits, uint32_t p) {
    const uint8_t* s = d + (p >> 3);
    const uint64_t w = (uint64_t)s[0] << 32 | (uint64_t)s[1] << 24 | (uint64_t)s[2] << 16 | (uint64_t)s[3] << 8 | (uint64_t)s[4];
    const uint32_t v = (uint32_t)(w >> (8 - (p & 7)));
    const uint32_t avail = bits - p;
    return avail >= 32 ? v : avail == 0 ? 0u : v & ~(0xffffffffu >> avail);
}

// the code at the head of v (32 bits, left aligned) -> length << 8 | symbol, 0: no code (huff_decode's two steps)
HPMVS_JPG_FN uint32_t huff_lookup(const Huff& h, uint32_t v) {
    const uint32_t e = h.lut[v >> 23];
    if (e >> 8) return e;
    for (int l = 10; l <= 16; l++) {
        const int32_t code = (int32_t)(v >> (32 - l));
        if (h.maxcode[l] >= 0 && code >= h.mincode[l] && code <= h.maxcode[l])
            return (uint32_t)l << 8 | h.vals[h.valptr[l] + code - h.mincode[l]];
    }
    return 0;
}

// receive_extend on the n bits (1 <= n <= 15) at the head of v
HPMVS_JPG_FN int32_t extend_bits(uint32_t v, int n) {
    const int32_t x = (int32_t)(v >> (32 - n));
    return x < (1 << (n - 1)) ? x - (1 << n) + 1 : x;
}

// Decodes the symbols of one segment that start in front of bit `end` (the subsequence's last bit + 1, at most the
// segment's length `bits`), from the entry state `in`.  tabs: per component the DC and the AC table ([2 c], [2 c + 1]).
// Every iteration consumes at least one bit or ends the loop: a symbol that the segment's remaining bits cannot hold is
// left unread (the padding behind the last block).  An invalid code with 16 bits in sight or k > 63 marks the exit with
// kStateErr, and the decoder goes on behind it (one bit on, or into the next block): a guess that stopped at its first
// error could never meet the true decode again, and every later subsequence would wait for a hand-over one by one.  The
// mark says that THIS decode of the subsequence met an error; it is not handed on (handed_on), and a chain is accepted
// only if none of its members carries it.  Exit state and counts are a function of the entry state and the bits alone.
// coef != nullptr: coefficients are stored as decode_scan stores them; the block in progress at entry is the segment's
// block number first_blk, blocks from seg_blocks on are dropped, and dc[] holds the predictions at entry.
HPMVS_JPG_FN SubState decode_subseq(const uint8_t* d, uint32_t bits, uint32_t end, const Huff* tabs, const ScanInfo& si,
                                    const uint8_t* zigzag, SubState in, SubCount* cnt, int16_t* coef, uint32_t first_blk,
                                    uint32_t seg_first_mcu, uint32_t seg_blocks, const uint32_t* dc_in) {
    uint32_t p = in.p, nblk = 0;
    uint32_t dc[3] = {0, 0, 0};
    if (dc_in) { dc[0] = dc_in[0]; dc[1] = dc_in[1]; dc[2] = dc_in[2]; }
    if (cnt) { cnt->nblk = 0; cnt->dc[0] = cnt->dc[1] = cnt->dc[2] = 0; }
    int blk = (int)(in.bk >> 8), k = (int)(in.bk & 63);
    bool err = false;
    int16_t* out = nullptr;  // the block in progress, where it is stored
    bool out_known = false;
    while (p < end) {
        const int c = si.blk_comp[blk];
        if (coef && !out_known) {
            const uint32_t g = first_blk + nblk;
            out = nullptr;
            if (g < seg_blocks) {
                const uint32_t mcu = seg_first_mcu + g / (uint32_t)si.bpm;
                if (mcu < (uint32_t)si.n_mcus) {
                    const uint32_t my = mcu / (uint32_t)si.mcus_x, mx = mcu - my * (uint32_t)si.mcus_x;
                    out = coef + si.off[c] + ((size_t)(my * si.v[c] + si.blk_dy[blk]) * si.bx[c] + (mx * si.h[c] + si.blk_dx[blk])) * 64;
                }
            }
            out_known = true;
        }
        const uint32_t v = peek32(d, bits, p);
        const uint32_t avail = bits - p;
        const uint32_t e = huff_lookup(tabs[2 * c + (k != 0)], v);
        const uint32_t len = e >> 8;
        if (len == 0) {
            if (avail < 16) break;
            err = true;  // no code: one bit on
            p++;
            continue;
        }
        const int sym = (int)(e & 255);
        const int sz = k == 0 ? sym : (sym & 15);  // (DC symbols are at most 15: parse_headers)
        if (len + (uint32_t)sz > avail) break;
        const uint32_t vv = sz ? peek32(d, bits, p + len) : 0u;
        bool done = false;
        if (k == 0) {
            const int32_t diff = sz ? extend_bits(vv, sz) : 0;
            dc[c] += (uint32_t)diff;
            if (out) out[0] = (int16_t)(int32_t)dc[c];
            k = 1;
        } else {
            const int r = sym >> 4;
            if (sz == 0) {
                if (r != 15) done = true;
                else k += 16;
            } else {
                k += r;
                if (k > 63) err = true;  // the block ends here
                else if (out) out[zigzag[k]] = (int16_t)extend_bits(vv, sz);
                k++;
            }
            if (k >= 64) done = true;
        }
        p += len + (uint32_t)sz;
        if (done) {
            k = 0;
            nblk++;
            blk = blk + 1 == si.bpm ? 0 : blk + 1;
            out_known = false;
        }
    }
    if (cnt) {
        cnt->nblk = nblk;
        for (int c = 0; c < 3; c++) cnt->dc[c] = dc[c] - (dc_in ? dc_in[c] : 0u);
    }
    SubState o;
    o.p = p;
    o.bk = (err ? kStateErr : 0u) | (uint32_t)blk << 8 | (uint32_t)k;
    return o;
}

// the guess a subsequence starts from: its first bit, block 0, the DC code next (for a segment's first one, the truth)
HPMVS_JPG_FN SubState guess_state(uint32_t index_in_segment, uint32_t subseq_bits) {
    SubState s;
    s.p = index_in_segment * subseq_bits;
    s.bk = 0;
    return s;
}

// What the check asks of a segment whose chain is consistent: no error, the last block just completed, exactly the
// segment's blocks, and fewer than 8 unread bits unless it is the scan's last segment (decode_scan leaves those unread
// too, but finds a restart marker only right behind the byte it stopped in).
HPMVS_JPG_FN bool segment_ok(const Segment& g, SubState last_exit, uint32_t blocks, int bpm, bool last_segment) {
    if (last_exit.bk != 0 || last_exit.p > g.bits) return false;
    if (blocks != g.n_mcus * (uint32_t)bpm) return false;
    return last_segment || g.bits - last_exit.p < 8;
}

// (plain C++ from here on)
struct Prescan {
    std::vector<uint8_t> bytes;  // the scan without its stuffing and markers, 16 zero bytes behind
    std::vector<Segment> segs;
    size_t n_subs = 0;
};

inline ScanInfo make_scan_info(const Frame& fr) {
    ScanInfo si;
    memset(&si, 0, sizeof(si));
    si.ncomp = fr.ncomp;
    si.mcus_x = fr.mcus_x;
    si.n_mcus = fr.mcus_x * fr.mcus_y;
    int b = 0;
    for (int c = 0; c < fr.ncomp; c++) {
        si.h[c] = fr.c[c].h; si.v[c] = fr.c[c].v; si.bx[c] = fr.c[c].bx;
        si.off[c] = (uint32_t)fr.c[c].off;
        for (int by = 0; by < fr.c[c].v; by++)
            for (int bx = 0; bx < fr.c[c].h; bx++, b++) {
                si.blk_comp[b] = (uint8_t)c; si.blk_dx[b] = (uint8_t)bx; si.blk_dy[b] = (uint8_t)by;
            }
    }
    si.bpm = b;
    return si;
}

// per component the DC and AC table the scan names, in the order decode_subseq indexes them
inline void scan_tables(const Frame& fr, const Huff* huff, Huff* tabs6) {
    for (int c = 0; c < 3; c++) {
        const int cc = c < fr.ncomp ? c : 0;
        tabs6[2 * c] = huff[fr.c[cc].td];
        tabs6[2 * c + 1] = huff[4 + fr.c[cc].ta];
    }
}

// Walks the scan's bytes once: drops the 00 of every FF 00, cuts at the RSTn markers the frame's restart interval
// expects (numbered 0, 1, .. mod 8) and stops at the first other marker, behind which EOI must come before any other
// scan.  false: something the parallel decode does not take on (FF FF fill, a restart marker too few, misnumbered or
// without a restart interval, no end marker, no EOI, 512 MiB of scan) -- decode_scan then decides what the file is.
inline bool prescan(const uint8_t* b, size_t n, size_t scan_start, const Frame& fr, Prescan& ps) {
    const size_t total_mcus = (size_t)fr.mcus_x * fr.mcus_y;
    const size_t interval = fr.restart ? (size_t)fr.restart : total_mcus;
    const size_t want = (total_mcus + interval - 1) / interval;  // segments
    if (n - scan_start >= ((size_t)1 << 29) || want >= ((size_t)1 << 28)) return false;
    ps.bytes.clear();
    ps.bytes.reserve(n - scan_start + 16);
    ps.segs.clear();
    size_t seg_first = 0, p = scan_start, end_marker = n;
    for (;;) {
        if (p >= n) return false;  // no marker ends the scan
        const uint8_t v = b[p];
        if (v != 0xFF) { ps.bytes.push_back(v); p++; continue; }
        if (p + 1 >= n) return false;
        const uint8_t m = b[p + 1];
        if (m == 0) { ps.bytes.push_back(0xFF); p += 2; continue; }
        if (m == 0xFF) return false;
        const bool rst = m >= 0xD0 && m <= 0xD7;
        const bool expected = rst && ps.segs.size() + 1 < want;  // (any marker ends the last segment, as it stops decode_scan)
        if (expected && m != 0xD0 + (ps.segs.size() & 7)) return false;
        Segment g;
        g.first_byte = (uint32_t)seg_first;
        g.bits = (uint32_t)((ps.bytes.size() - seg_first) * 8);
        g.first_mcu = (uint32_t)(ps.segs.size() * interval);
        g.n_mcus = (uint32_t)(total_mcus - g.first_mcu < interval ? total_mcus - g.first_mcu : interval);
        g.first_sub = g.n_subs = 0;
        ps.segs.push_back(g);
        seg_first = ps.bytes.size();
        if (!expected) { end_marker = p; break; }
        p += 2;
    }
    if (ps.segs.size() != want) return false;
    ps.bytes.insert(ps.bytes.end(), 16, 0);
    for (size_t q = end_marker; q + 1 < n; q++) {  // decode_scan's search behind the scan
        if (b[q] != 0xFF) continue;
        if (b[q + 1] == 0xD9) return true;
        if (b[q + 1] == 0xDA) return false;
    }
    return false;
}

// cuts every segment into subsequences of subseq_bits (one at least) -> their number
inline size_t plan_subsequences(Prescan& ps, uint32_t subseq_bits) {
    size_t n = 0;
    for (Segment& g : ps.segs) {
        g.first_sub = (uint32_t)n;
        g.n_subs = g.bits ? (g.bits + subseq_bits - 1) / subseq_bits : 1;
        n += g.n_subs;
    }
    ps.n_subs = n;
    return n;
}

}  // namespace jpg
}  // namespace hpmvs
