// jpeg_enc.hpp -- baseline JPEG encoding of a view's level (reference Scene::saveAsNVM through CImg's save_jpeg and
// libjpeg's defaults, src/hpmvs/Scene.cpp:646-713: jpeg_set_defaults + jpeg_set_quality(q, TRUE) on RGB rows, i.e. YCbCr
// 4:2:0, JDCT_ISLOW, the Annex K Huffman tables, no restart markers), written once for the device kernels
// (kernel_jpeg_encode.hip), the C ABI (capi_image.hip) and the host restatement the tests compile with g++
// (tests/jpeg_enc_host.cpp).  Everything is integer arithmetic; the file it describes equals libjpeg's byte for byte.
//
// The split: per MCU (Y00 Y01 Y10 Y11 Cb Cr) colour conversion, edge replication, h2v2 downsampling, the forward DCT and
// the quantiser give six blocks of int16 coefficients in zigzag order; encode_block walks one block into (code, length)
// pairs that a sink counts or writes; the byte stream is stuffed behind that and the host puts write_header in front.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define HPMVS_JPGE_FN __host__ __device__ inline
#else
#define HPMVS_JPGE_FN inline
#endif

namespace hpmvs {
namespace jpge {

constexpr int kOk = 0, kErrArg = -2, kErrUnsupported = -5;  // HPMVS_OK, HPMVS_ERR_ARG, HPMVS_ERR_UNSUPPORTED
constexpr int kMinSide = 8, kMaxSide = 65535;               // the decoder's lower bound; SOF0's 16-bit fields
constexpr size_t kHeaderBytes = 623;                        // SOI .. SOS, see write_header
// A block's code is at most a DC of 11 + 11 bits and 63 ACs of 16 + 10 bits: 1660 bits, under 208 bytes.
constexpr size_t kBlockBoundBytes = 208;

// ------------------------------------------------------------------------------------------------ geometry
struct Geom {
    int32_t W, H;
    int32_t mcux, mcuy;  // 16 x 16 MCUs
    int32_t bw, bh;      // luma blocks that hold image samples: ceil(W / 8), ceil(H / 8); the others are dummy blocks
    int32_t ch;          // chroma rows that hold image samples: ceil(H / 2)
    uint32_t n_blocks;   // 6 per MCU, in scan order
};

HPMVS_JPGE_FN Geom make_geom(int W, int H) {
    Geom g;
    g.W = W; g.H = H;
    g.mcux = (W + 15) / 16; g.mcuy = (H + 15) / 16;
    g.bw = (W + 7) / 8; g.bh = (H + 7) / 8;
    g.ch = (H + 1) / 2;
    g.n_blocks = 6u * (uint32_t)g.mcux * (uint32_t)g.mcuy;
    return g;
}

// Block b of the scan (6 m + i): the block its DC is predicted from, -1 for a component's first block.  Luma follows the
// luma block before it in scan order (Y11 of the MCU before for Y00), chroma the same component of the MCU before.
HPMVS_JPGE_FN int64_t dc_predecessor(uint32_t b) {
    const uint32_t i = b % 6u;
    if (i >= 1 && i <= 3) return (int64_t)b - 1;
    if (b < 6) return -1;
    return i == 0 ? (int64_t)b - 3 : (int64_t)b - 6;
}

// upper bound of the whole file: every block at its worst, every byte of the entropy data stuffed, the pad byte, EOI
inline size_t encode_bound(int W, int H) {
    const size_t blocks = (size_t)6 * (size_t)((W + 15) / 16) * (size_t)((H + 15) / 16);
    return kHeaderBytes + 2 * (kBlockBoundBytes * blocks + 1) + 2;
}

// ------------------------------------------------------------------------------------------------ per-sample arithmetic
constexpr int32_t fix16(double x) { return (int32_t)(x * 65536.0 + 0.5); }

// libjpeg's rgb_ycc_convert: 16-bit fixed point, the chroma rounding one below a half
HPMVS_JPGE_FN void rgb_to_ycc(int r, int g, int b, int* y, int* cb, int* cr) {
    constexpr int32_t kHalf = 32768, kOff = 128 << 16;
    *y = (fix16(0.299) * r + fix16(0.587) * g + fix16(0.114) * b + kHalf) >> 16;
    *cb = (-fix16(0.16874) * r - fix16(0.33126) * g + fix16(0.5) * b + kOff + kHalf - 1) >> 16;
    *cr = (fix16(0.5) * r - fix16(0.41869) * g - fix16(0.08131) * b + kOff + kHalf - 1) >> 16;
}

// h2v2_downsample: the bias alternates 1, 2 along the output row
HPMVS_JPGE_FN int h2v2(int a, int b, int c, int d, int out_col) { return (a + b + c + d + 1 + (out_col & 1)) >> 2; }

HPMVS_JPGE_FN int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2).  Pass 1 runs along the rows of the samples minus 128
// and leaves its results scaled up by 4; pass 2 runs down the columns of that and takes the 4 out again.  The two passes
// together leave the factor 8 the quantiser divides by.
HPMVS_JPGE_FN void fdct_1d(const int32_t* d, int32_t* o, bool pass2) {
    int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = pass2 ? 13 + 2 : 13 - 2;
    if (pass2) {
        o[0] = descale(t10 + t11, 2);
        o[4] = descale(t10 - t11, 2);
    } else {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    }
    int32_t z1 = (t12 + t13) * 4433;
    o[2] = descale(z1 + t13 * 6270, sh);
    o[6] = descale(z1 - t12 * 15137, sh);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    o[7] = descale(t4 + z1 + z3, sh);
    o[5] = descale(t5 + z2 + z4, sh);
    o[3] = descale(t6 + z2 + z3, sh);
    o[1] = descale(t7 + z1 + z4, sh);
}

// forward_DCT's quantiser: q8 = 8 * the table's step (the DCT's factor), rounded half away from zero
HPMVS_JPGE_FN int16_t quantize(int32_t c, int32_t q8) {
    const int32_t a = c < 0 ? -c : c;
    const int32_t v = (a + (q8 >> 1)) / q8;
    return (int16_t)(c < 0 ? -v : v);
}

// The DCs of an MCU's four luma blocks behind the dummy rule: a dummy block (bit i of `dummy`) takes the quantised DC of the
// block before it in the MCU.  Y00 is never a dummy.
HPMVS_JPGE_FN void fill_dummy_dc(int16_t* dc, int dummy) {
    for (int i = 1; i < 4; i++)
        if (dummy >> i & 1) dc[i] = dc[i - 1];
}

// bit i: luma block i of MCU (mx, my) lies beyond the blocks that hold image samples
HPMVS_JPGE_FN int dummy_mask(const Geom& g, int mx, int my) {
    int m = 0;
    for (int i = 0; i < 4; i++)
        if (2 * mx + (i & 1) >= g.bw || 2 * my + (i >> 1) >= g.bh) m |= 1 << i;
    return m;
}

// ------------------------------------------------------------------------------------------------ tables the kernels read
// (built by make_tables on the host; the kernels copy them to LDS)
struct EncTables {
    uint16_t q8[2][64];        // 8 * quantiser step, luma / chroma, in zigzag order
    uint16_t dc_code[2][16];
    uint16_t ac_code[2][256];
    uint8_t dc_len[2][16];
    uint8_t ac_len[2][256];
    uint8_t zz[64];            // natural position of zigzag index k
};
static_assert(sizeof(EncTables) % 4 == 0, "the tables are copied to LDS in words");

HPMVS_JPGE_FN int bit_length(uint32_t t) { return t ? 32 - __builtin_clz(t) : 0; }

// One block -> its symbols: sink.put(code, length) per Huffman code and per run of appended bits, in stream order; the
// sink also hears what the test fixtures count (dc_category, zrl).  zz: 64 coefficients in zigzag order, pred: the DC of
// dc_predecessor, tab: 0 luma, 1 chroma.
template <class Sink>
HPMVS_JPGE_FN void encode_block(const int16_t* zz, int pred, const EncTables& T, int tab, Sink& sink) {
    int v = (int)zz[0] - pred;
    int n = bit_length((uint32_t)(v < 0 ? -v : v));
    sink.put(T.dc_code[tab][n], T.dc_len[tab][n]);
    if (n) sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
    sink.dc_category(n);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        v = zz[k];
        if (v == 0) { run++; continue; }
        while (run > 15) {
            sink.put(T.ac_code[tab][0xF0], T.ac_len[tab][0xF0]);
            sink.zrl();
            run -= 16;
        }
        n = bit_length((uint32_t)(v < 0 ? -v : v));
        const int sym = run << 4 | n;
        sink.put(T.ac_code[tab][sym], T.ac_len[tab][sym]);
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
        run = 0;
    }
    if (run > 0) sink.put(T.ac_code[tab][0], T.ac_len[tab][0]);
}

struct LengthSink {
    uint32_t bits = 0;
    HPMVS_JPGE_FN void put(uint32_t, int n) { bits += (uint32_t)n; }
    HPMVS_JPGE_FN void dc_category(int) {}
    HPMVS_JPGE_FN void zrl() {}
};

// ------------------------------------------------------------------------------------------------ host: tables and header
static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K.1, K.2 (natural order)
static const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: codes per length 1 .. 16, then the symbols in code order.  Order: DC luma, AC luma, DC chroma, AC chroma.
static const uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t kHuffDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kHuffAcLuma[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kHuffAcChroma[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

inline const uint8_t* huff_vals(int t, int* n) {
    *n = (t & 1) ? 162 : 12;
    return t == 1 ? kHuffAcLuma : t == 3 ? kHuffAcChroma : kHuffDcVals;
}

// jpeg_set_quality(q, TRUE): the step of table t (0 luma, 1 chroma) at natural position k
inline int quant_step(int t, int k, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (kBaseQ[t][k] * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// what the C ABI refuses, with its reason
inline int check_args(int W, int H, int quality, std::string* err) {
    if (quality < 1 || quality > 100) { if (err) *err = "jpeg_encode: quality must be 1 .. 100"; return kErrArg; }
    if (W > kMaxSide || H > kMaxSide) { if (err) *err = "jpeg_encode: a side above 65535 pixels does not fit a JPEG frame header"; return kErrArg; }
    if (W < kMinSide || H < kMinSide) { if (err) *err = "jpeg_encode: a side under 8 pixels is below what the decoder here reads back"; return kErrUnsupported; }
    return kOk;
}

inline void make_tables(int quality, EncTables* T) {
    memset(T, 0, sizeof(*T));
    for (int k = 0; k < 64; k++) {
        T->zz[k] = kZigzag[k];
        for (int t = 0; t < 2; t++) T->q8[t][k] = (uint16_t)(8 * quant_step(t, kZigzag[k], quality));
    }
    for (int t = 0; t < 4; t++) {  // Annex C: codes in order of length, counting up
        int n = 0;
        const uint8_t* vals = huff_vals(t, &n);
        uint32_t code = 0;
        int at = 0;
        for (int len = 1; len <= 16; len++) {
            for (int j = 0; j < kHuffBits[t][len - 1]; j++, at++, code++) {
                const int sym = vals[at];
                if (t & 1) { T->ac_code[t >> 1][sym] = (uint16_t)code; T->ac_len[t >> 1][sym] = (uint8_t)len; }
                else { T->dc_code[t >> 1][sym] = (uint16_t)code; T->dc_len[t >> 1][sym] = (uint8_t)len; }
            }
            code <<= 1;
        }
    }
}

// SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS: kHeaderBytes bytes at `o`
inline void write_header(int W, int H, int quality, uint8_t* o) {
    auto u8 = [&o](int v) { *o++ = (uint8_t)v; };
    auto u16 = [&o](int v) { *o++ = (uint8_t)(v >> 8); *o++ = (uint8_t)v; };
    u16(0xFFD8);
    u16(0xFFE0); u16(16);
    for (const char c : {'J', 'F', 'I', 'F', '\0'}) u8(c);
    u16(0x0101); u8(0); u16(1); u16(1); u8(0); u8(0);
    for (int t = 0; t < 2; t++) {
        u16(0xFFDB); u16(67); u8(t);
        for (int k = 0; k < 64; k++) u8(quant_step(t, kZigzag[k], quality));
    }
    u16(0xFFC0); u16(17); u8(8); u16(H); u16(W); u8(3);
    u8(1); u8(0x22); u8(0);
    u8(2); u8(0x11); u8(1);
    u8(3); u8(0x11); u8(1);
    for (int t = 0; t < 4; t++) {
        int n = 0;
        const uint8_t* vals = huff_vals(t, &n);
        u16(0xFFC4); u16(19 + n); u8((t & 1) << 4 | t >> 1);
        for (int k = 0; k < 16; k++) u8(kHuffBits[t][k]);
        for (int k = 0; k < n; k++) u8(vals[k]);
    }
    u16(0xFFDA); u16(12); u8(3);
    u8(1); u8(0x00);
    u8(2); u8(0x11);
    u8(3); u8(0x11);
    u8(0); u8(63); u8(0);
}

}  // namespace jpge
}  // namespace hpmvs
