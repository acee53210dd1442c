// Host restatement of the baseline JPEG decode: the product's parser, entropy decoder and per-block / per-pixel
// arithmetic (hpmvs_amd/csrc/jpeg.hpp, the functions kernel_jpeg.hip calls) compiled by g++ and run in plain loops.
// tests/test_cpu_jpeg.py pins it to Pillow's (libjpeg-turbo's) pixels byte for byte (tests/golden/g7_jpeg.npz); the GPU
// tests and tools/jpeg_scale.py compare the kernels with it.  Build: g++ -std=c++14 -O2 -fPIC -shared jpeg_host.cpp
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../hpmvs_amd/csrc/jpeg.hpp"

using namespace hpmvs::jpg;

static void put_err(const std::string& e, char* err, int cap) {
    if (err && cap > 0) snprintf(err, (size_t)cap, "%s", e.c_str());
}

// coefficients -> sample planes: per block dequantise, column pass, row pass, range limit
static void idct_planes(const Frame& fr, const Planes& P, uint8_t* planes) {
    for (int c = 0; c < fr.ncomp; c++) {
        const Component& C = fr.c[c];
        for (int by = 0; by < C.by; by++)
            for (int bx = 0; bx < C.bx; bx++) {
                const int16_t* blk = &fr.coef[C.off + ((size_t)by * C.bx + bx) * 64];
                int32_t ws[8][8], in[8], out[8];
                for (int col = 0; col < 8; col++) {
                    for (int r = 0; r < 8; r++) in[r] = dequant(blk[r * 8 + col], fr.q[c][r * 8 + col]);
                    idct_1d(in, out, kPass1Shift);
                    for (int r = 0; r < 8; r++) ws[r][col] = out[r];
                }
                for (int r = 0; r < 8; r++) {
                    idct_1d(ws[r], out, kPass2Shift);
                    uint8_t* o = planes + P.off[c] + ((size_t)by * 8 + r) * P.stride[c] + bx * 8;
                    for (int k = 0; k < 8; k++) o[k] = range_limit(out[k]);
                }
            }
    }
}

extern "C" {

int jh_info(const uint8_t* bytes, size_t n, int* w, int* h, int* comps, int* hs, int* vs, char* err, int errcap) {
    Frame fr;
    std::string e;
    const int rc = decode_file(bytes, n, fr, false, &e);
    put_err(e, err, errcap);
    if (rc != kOk) return rc;
    *w = fr.W; *h = fr.H; *comps = fr.ncomp; *hs = fr.hmax; *vs = fr.vmax;
    return kOk;
}

// counts[k]: blocks of the file whose coefficient at natural position k is not 0 (what a fixture file exercises)
int jh_nonzero_positions(const uint8_t* bytes, size_t n, uint32_t* counts) {
    Frame fr;
    const int rc = decode_file(bytes, n, fr, true, nullptr);
    if (rc != kOk) return rc;
    for (int k = 0; k < 64; k++) counts[k] = 0;
    for (size_t i = 0; i < fr.coef.size(); i++) counts[i & 63] += fr.coef[i] != 0;
    return kOk;
}

// rgb: interleaved u8 [H][W][3]; exactly 3 W H bytes are written
int jh_decode(const uint8_t* bytes, size_t n, uint8_t* rgb, size_t cap, char* err, int errcap) {
    Frame fr;
    std::string e;
    const int rc = decode_file(bytes, n, fr, true, &e);
    put_err(e, err, errcap);
    if (rc != kOk) return rc;
    if (cap < (size_t)3 * fr.W * fr.H) {
        put_err("jpeg: output buffer too small", err, errcap);
        return kErrArg;
    }
    Planes P;
    std::vector<uint8_t> planes(make_planes(fr, &P));
    idct_planes(fr, P, planes.data());
    for (int y = 0; y < fr.H; y++)
        for (int x0 = 0; x0 < fr.W; x0 += 4) {
            uint8_t px[12];
            convert_quad(planes.data(), P, x0, y, px);
            const int nb = 3 * (fr.W - x0 < 4 ? fr.W - x0 : 4);
            uint8_t* o = rgb + 3 * ((size_t)y * fr.W + x0);
            for (int k = 0; k < nb; k++) o[k] = px[k];
        }
    return kOk;
}

}  // extern "C"
