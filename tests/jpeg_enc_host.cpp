// Host restatement of the baseline JPEG encode: the product's tables, per-sample arithmetic, block walk and header
// writer (hpmvs_amd/csrc/jpeg_enc.hpp, the functions kernel_jpeg_encode.hip calls) compiled by g++ and run in plain
// loops, one MCU and one block after the other, with a sequential bit writer.  tests/test_cpu_jpeg_encode.py pins it to
// Pillow's (libjpeg-turbo's) files byte for byte (tests/golden/g8_jpeg_enc.npz); the GPU tests compare the kernels with
// the same files.  Build: g++ -std=c++14 -O2 -fPIC -shared jpeg_enc_host.cpp   (-DJPEG_ENC_HOST_MAIN: a program that
// encodes the raw cases of a file made by tests/golden/make_golden_jpeg_enc.py --dump, for a sanitizer run)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../hpmvs_amd/csrc/jpeg_enc.hpp"

using namespace hpmvs::jpge;

static int imin(int a, int b) { return a < b ? a : b; }

// The six blocks of MCU (mx, my), quantised, in zigzag order.  Edges: luma and the full-size chroma planes repeat the last
// column and the last row (the chroma planes only up to an even number of rows, which the clamp gives as well); chroma rows
// below the last one that holds image samples repeat that DOWNSAMPLED row.
static void mcu_blocks(const uint8_t* rgb, const Geom& g, const EncTables& T, int mx, int my, int16_t out[6][64]) {
    int Y[16][16], Cb[16][16], Cr[16][16], C[2][8][8];
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) {
            const uint8_t* p = rgb + 3 * ((size_t)imin(16 * my + y, g.H - 1) * g.W + imin(16 * mx + x, g.W - 1));
            rgb_to_ycc(p[0], p[1], p[2], &Y[y][x], &Cb[y][x], &Cr[y][x]);
        }
    for (int cy = 0; cy < 8; cy++) {
        const int sy = imin(8 * my + cy, g.ch - 1) - 8 * my;  // the chroma row it repeats, inside this MCU
        for (int cx = 0; cx < 8; cx++) {
            C[0][cy][cx] = h2v2(Cb[2 * sy][2 * cx], Cb[2 * sy][2 * cx + 1], Cb[2 * sy + 1][2 * cx], Cb[2 * sy + 1][2 * cx + 1], cx);
            C[1][cy][cx] = h2v2(Cr[2 * sy][2 * cx], Cr[2 * sy][2 * cx + 1], Cr[2 * sy + 1][2 * cx], Cr[2 * sy + 1][2 * cx + 1], cx);
        }
    }
    for (int b = 0; b < 6; b++) {
        int32_t in[8], ws[8][8], col[8], res[8], nat[64];
        for (int r = 0; r < 8; r++) {
            for (int k = 0; k < 8; k++) in[k] = (b < 4 ? Y[8 * (b >> 1) + r][8 * (b & 1) + k] : C[b - 4][r][k]) - 128;
            fdct_1d(in, ws[r], false);
        }
        for (int c = 0; c < 8; c++) {
            for (int r = 0; r < 8; r++) col[r] = ws[r][c];
            fdct_1d(col, res, true);
            for (int r = 0; r < 8; r++) nat[8 * r + c] = res[r];
        }
        for (int k = 0; k < 64; k++) out[b][k] = quantize(nat[T.zz[k]], T.q8[b < 4 ? 0 : 1][k]);
    }
    const int dummy = dummy_mask(g, mx, my);
    int16_t dc[4] = {out[0][0], out[1][0], out[2][0], out[3][0]};
    fill_dummy_dc(dc, dummy);
    for (int i = 1; i < 4; i++)
        if (dummy >> i & 1) {
            for (int k = 1; k < 64; k++) out[i][k] = 0;
            out[i][0] = dc[i];
        }
}

// MSB-first bit writer with byte stuffing, and the counts the fixture script asserts on
struct ByteSink {
    std::vector<uint8_t>& o;
    uint32_t acc = 0;
    int fill = 0;
    uint32_t stuffed = 0, zrls = 0, dc_cat_max = 0, pad_bits = 0;
    explicit ByteSink(std::vector<uint8_t>& out) : o(out) {}
    void byte(uint8_t b) {
        o.push_back(b);
        if (b == 0xFF) { o.push_back(0); stuffed++; }
    }
    void put(uint32_t code, int n) {
        for (int k = n - 1; k >= 0; k--) {
            acc = acc << 1 | (code >> k & 1u);
            if (++fill == 8) { byte((uint8_t)acc); acc = 0; fill = 0; }
        }
    }
    void dc_category(int n) { if ((uint32_t)n > dc_cat_max) dc_cat_max = (uint32_t)n; }
    void zrl() { zrls++; }
    void finish() {
        pad_bits = fill ? 8 - fill : 0;
        if (fill) put((1u << pad_bits) - 1u, (int)pad_bits);
    }
};

// stats (nullable): [0] stuffed bytes, [1] 0xF0 symbols, [2] largest DC category, [3] pad bits, [4] right-edge dummy
// blocks, [5] bottom-row dummy blocks
static int encode(const uint8_t* rgb, int W, int H, int quality, std::vector<uint8_t>& file, uint32_t* stats, std::string* err) {
    const int rc = check_args(W, H, quality, err);
    if (rc != kOk) return rc;
    const Geom g = make_geom(W, H);
    EncTables T;
    make_tables(quality, &T);
    std::vector<int16_t> coef((size_t)g.n_blocks * 64);
    uint32_t right = 0, bottom = 0;
    for (int my = 0; my < g.mcuy; my++)
        for (int mx = 0; mx < g.mcux; mx++) {
            mcu_blocks(rgb, g, T, mx, my, reinterpret_cast<int16_t(*)[64]>(&coef[((size_t)my * g.mcux + mx) * 6 * 64]));
            const int d = dummy_mask(g, mx, my);
            right += (d >> 1 & 1) && 2 * my < g.bh && 2 * mx + 1 >= g.bw;
            bottom += (d >> 2 & 1) && 2 * my + 1 >= g.bh;
        }
    file.assign(kHeaderBytes, 0);
    write_header(W, H, quality, file.data());
    ByteSink sink(file);
    for (uint32_t b = 0; b < g.n_blocks; b++) {
        const int64_t p = dc_predecessor(b);
        encode_block(&coef[(size_t)b * 64], p < 0 ? 0 : coef[(size_t)p * 64], T, b % 6 < 4 ? 0 : 1, sink);
    }
    sink.finish();
    file.push_back(0xFF);
    file.push_back(0xD9);
    if (stats) {
        stats[0] = sink.stuffed; stats[1] = sink.zrls; stats[2] = sink.dc_cat_max; stats[3] = sink.pad_bits;
        stats[4] = right; stats[5] = bottom;
    }
    return kOk;
}

extern "C" {

size_t je_bound(int W, int H) { return encode_bound(W, H); }

// rgb: interleaved u8 [H][W][3].  *n: the file's length, also when cap is too small (kErrArg; nothing is written then)
int je_encode(const uint8_t* rgb, int W, int H, int quality, uint8_t* out, size_t cap, size_t* n, uint32_t* stats, char* err, int errcap) {
    std::vector<uint8_t> file;
    std::string e;
    int rc = encode(rgb, W, H, quality, file, stats, &e);
    if (rc == kOk) {
        *n = file.size();
        if (cap < file.size()) { rc = kErrArg; e = "jpeg_encode: output buffer too small"; }
        else for (size_t k = 0; k < file.size(); k++) out[k] = file[k];
    }
    if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", e.c_str());
    return rc;
}

}  // extern "C"

#ifdef JPEG_ENC_HOST_MAIN
// cases file: per case int32 W, H, quality, then 3 W H bytes; writes nothing, prints one line per case
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[3];
    int cases = 0;
    while (fread(hd, 4, 3, f) == 3) {
        std::vector<uint8_t> rgb((size_t)3 * hd[0] * hd[1]);
        if (fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 3;
        std::vector<uint8_t> out(je_bound(hd[0], hd[1]));
        size_t n = 0;
        uint32_t stats[6];
        const int rc = je_encode(rgb.data(), hd[0], hd[1], hd[2], out.data(), out.size(), &n, stats, nullptr, 0);
        if (rc != kOk || n > out.size()) { printf("case %d: rc %d\n", cases, rc); return 1; }
        unsigned sum = 0;
        for (size_t k = 0; k < n; k++) sum = sum * 31u + out[k];
        printf("case %d: %dx%d q%d -> %zu bytes, hash %08x\n", cases, hd[0], hd[1], hd[2], n, sum);
        cases++;
    }
    fclose(f);
    // the refusals and a buffer that is one byte short
    std::vector<uint8_t> px(3 * 16 * 16, 7), out(je_bound(16, 16));
    size_t n = 0;
    if (je_encode(px.data(), 16, 16, 0, out.data(), out.size(), &n, nullptr, nullptr, 0) != kErrArg) return 1;
    if (je_encode(px.data(), 7, 16, 90, out.data(), out.size(), &n, nullptr, nullptr, 0) != kErrUnsupported) return 1;
    if (je_encode(px.data(), 16, 16, 90, out.data(), out.size(), &n, nullptr, nullptr, 0) != kOk) return 1;
    std::vector<uint8_t> tight(n - 1);
    if (je_encode(px.data(), 16, 16, 90, tight.data(), tight.size(), &n, nullptr, nullptr, 0) != kErrArg) return 1;
    printf("%d cases ok\n", cases);
    return 0;
}
#endif
