// capi_image.hip -- the image entry points of include/hpmvs_amd.h: baseline JPEG decode (host walk or device entropy decode)
// and encode, radial undistortion, the stand-alone pyramid step and the depth maps as jet-coloured images.  Only the last
// reach into a scene, through scene_depth_maps of capi_common.hpp; the scene entries of capi.hip that take or give JPEG bytes
// call the functions capi_common.hpp declares.  Host-side only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hpmvs_amd.h"
#include "capi_common.hpp"
#include "depth_vis.hpp"
#include "dev_types.h"
#include "launch.h"

using namespace hpmvs;
using namespace hpmvs::capi;

// ---- baseline JPEG (jpeg.hpp: the host parses; the scan is entropy-decoded by the host walk or, checked, by
// kernel_jpeg_entropy.hip; kernel_jpeg.hip does the rest)
static int jpeg_fail(int code, const std::string& msg) { return fail(code == jpg::kErrUnsupported ? HPMVS_ERR_UNSUPPORTED : HPMVS_ERR_ARG, msg); }

constexpr size_t kJpegQBytes = sizeof(uint16_t) * 3 * 64;  // the quantiser steps in front of the coefficients in JpegFile::d_coef

// hpmvs_jpeg_last_decode: what decoded the scan in this thread's last successful JPEG decode
static thread_local int t_jpeg_last_used = -1, t_jpeg_last_rounds = 0;

// The scan decoded on the current device (kernel_jpeg_entropy.hip) into jf.d_coef, on the null stream.  *why stays empty when
// the check kernel accepted the chain; otherwise it says why the scan is the host walk's.  jf holds the device buffer only
// when the chain was accepted: on every other way out, an error included, the buffer is freed here.
// Working buffers the device cannot allocate leave the scan to the host walk like any other reason.
// ms (diagnostics, nullable): [0] prescan (wall clock); by HIP events [1] uploads and fills, [2] jpeg_entropy_sync_kernel, all
// passes, [3] the passes with their read-backs, [4] _scan_local, [5] _scan_groups, [6] _check, [7] _write kernel.
static int jpeg_entropy_device(JpegFile& jf, uint32_t subseq_bits, std::string* why, float* ms) {
    const jpg::Frame& fr = jf.fr;
    jpg::Prescan ps;
    const auto t0 = std::chrono::steady_clock::now();
    const bool taken = jpg::prescan(jf.bytes, jf.n, jf.scan_start, fr, ps);
    if (ms) ms[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!taken) {
        *why = "jpeg: the scan is not one the device decodes (fill bytes, restart markers or the end of the scan)";
        return HPMVS_OK;
    }
    const size_t n_subs = jpg::plan_subsequences(ps, subseq_bits);
    if (n_subs >= ((size_t)1 << 30)) { *why = "jpeg: too many subsequences"; return HPMVS_OK; }
    std::vector<uint32_t> sub_seg(n_subs);
    for (size_t s = 0; s < ps.segs.size(); s++)
        for (uint32_t i = 0; i < ps.segs[s].n_subs; i++) sub_seg[ps.segs[s].first_sub + i] = (uint32_t)s;
    std::vector<uint32_t> tabs((6 * sizeof(jpg::Huff) + 64) / 4);
    {
        std::vector<jpg::Huff> six(6);
        jpg::scan_tables(fr, jf.huff.data(), six.data());
        memcpy(tabs.data(), six.data(), 6 * sizeof(jpg::Huff));
        memcpy(tabs.data() + 6 * sizeof(jpg::Huff) / 4, jpg::kZigzag, 64);
    }
    JpegEntropy A;
    A.si = jpg::make_scan_info(fr);
    A.subseq_bits = subseq_bits;
    A.n_subs = (uint32_t)n_subs;
    A.n_segs = (uint32_t)ps.segs.size();
    A.n_groups = (uint32_t)((n_subs + jpg::kSubsPerGroup - 1) / jpg::kSubsPerGroup);
    A.n_scan_groups = (uint32_t)((n_subs + 255) / 256);
    Layout L;  // one working buffer
    const size_t o_bytes = L.take(ps.bytes.size()), o_segs = L.take(ps.segs.size() * sizeof(jpg::Segment)), o_sub = L.take(n_subs * 4),
                 o_tabs = L.take(tabs.size() * 4), o_entry = L.take(n_subs * sizeof(jpg::SubState)), o_exit = L.take(n_subs * sizeof(jpg::SubState)),
                 o_gexit = L.take((size_t)2 * A.n_groups * sizeof(jpg::SubState)), o_cnt = L.take(n_subs * sizeof(uint4)),
                 o_incl = L.take(n_subs * sizeof(uint4)), o_grp = L.take((size_t)A.n_scan_groups * sizeof(uint4)), o_flags = L.take(16);
    DeviceBuffer work_buf, coef_buf;  // (the coefficients become jf's only behind the check)
    const size_t coef_bytes = fr.n_blocks * 64 * sizeof(int16_t);
    if (work_buf.alloc(L.total) != hipSuccess || coef_buf.alloc(kJpegQBytes + coef_bytes) != hipSuccess) {
        (void)hipGetLastError();  // the failed allocation is no error of the call
        *why = "jpeg: no device memory for the entropy decode's working buffers";
        return HPMVS_OK;
    }
    uint8_t* const work = work_buf.p;
    int16_t* const d_coef = (int16_t*)(coef_buf.p + kJpegQBytes);
    A.bytes = work + o_bytes;
    A.segs = (const jpg::Segment*)(work + o_segs);
    A.sub_seg = (const uint32_t*)(work + o_sub);
    A.tabs = (const uint32_t*)(work + o_tabs);
    A.entry = (jpg::SubState*)(work + o_entry);
    A.exit = (jpg::SubState*)(work + o_exit);
    A.grp_exit = (jpg::SubState*)(work + o_gexit);
    A.cnt = (uint4*)(work + o_cnt);
    A.incl = (uint4*)(work + o_incl);
    A.grp = (uint4*)(work + o_grp);
    A.flags = (uint32_t*)(work + o_flags);
    // events: 0 start, 1 uploaded, 2 passes done, 3 .. 7 around the four kernels of the finish, 8 / 9 around a pass's kernel
    EventMarks ev(10, ms != nullptr);
    HIPCHK(ev.created());
    HIPCHK(ev.mark(0));
    if (ms) ms[2] = 0.0f;
    HIPCHK(hipMemcpy(work + o_bytes, ps.bytes.data(), ps.bytes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(work + o_segs, ps.segs.data(), ps.segs.size() * sizeof(jpg::Segment), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(work + o_sub, sub_seg.data(), n_subs * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(work + o_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(work + o_gexit, 0, (size_t)2 * A.n_groups * sizeof(jpg::SubState), nullptr));
    HIPCHK(hipMemsetAsync(work + o_flags, 0, 16, nullptr));
    HIPCHK(hipMemsetAsync(d_coef, 0, coef_bytes, nullptr));
    HIPCHK(ev.mark(1));
    const int cap = jpg::sync_round_cap(subseq_bits);
    int rounds = 0;
    bool out_of_rounds = false;
    for (int pass = 0;; pass++) {  // every pass but the last takes a round at least: at most cap + 2 passes
        HIPCHK(hipMemsetAsync(A.flags, 0, 8, nullptr));
        HIPCHK(ev.mark(8));
        launch_jpeg_entropy_sync(A, pass, cap - rounds, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(ev.mark(9));
        uint32_t f[2] = {0, 0};
        HIPCHK(hipMemcpy(f, A.flags, 8, hipMemcpyDeviceToHost));
        if (ms) {
            float t = 0.0f;
            HIPCHK(ev.elapsed(8, 9, &t));
            ms[2] += t;
        }
        rounds += (int)f[0];
        if (f[1]) { out_of_rounds = true; break; }
        if (pass > 0 && f[0] == 0) break;
    }
    jf.rounds = rounds;
    HIPCHK(ev.mark(2));
    uint32_t refused = 1;
    if (!out_of_rounds) {
        HIPCHK(launch_jpeg_entropy_finish(A, d_coef, nullptr, ev.from(3)));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&refused, A.flags + 2, 4, hipMemcpyDeviceToHost));
        if (ms) {
            HIPCHK(ev.elapsed(0, 1, &ms[1]));
            HIPCHK(ev.elapsed(1, 2, &ms[3]));
            for (int k = 0; k < 4; k++) HIPCHK(ev.elapsed(3 + k, 4 + k, &ms[4 + k]));
        }
    }
    if (refused) {
        *why = out_of_rounds ? "jpeg: the subsequences did not synchronise within " + std::to_string(cap) + " rounds"
                             : "jpeg: the check refused the chain of subsequences (corrupt entropy data, or data behind the last block)";
        return HPMVS_OK;
    }
    jf.d_coef = std::move(coef_buf);
    jf.used = HPMVS_JPEG_ENTROPY_DEVICE;  // (the quantiser steps in front of the coefficients: jpeg_frame_to_device)
    return HPMVS_OK;
}

namespace hpmvs {
namespace capi {

// HPMVS_JPEG_ENTROPY=host|device|auto, read once per process
int jpeg_entropy_env() {
    static const int mode = [] {
        const char* e = getenv("HPMVS_JPEG_ENTROPY");
        return e && !strcmp(e, "host") ? HPMVS_JPEG_ENTROPY_HOST : e && !strcmp(e, "device") ? HPMVS_JPEG_ENTROPY_DEVICE : HPMVS_JPEG_ENTROPY_AUTO;
    }();
    return mode;
}
bool jpeg_entropy_ok(int e) { return e == HPMVS_JPEG_ENTROPY_AUTO || e == HPMVS_JPEG_ENTROPY_HOST || e == HPMVS_JPEG_ENTROPY_DEVICE; }

int jpeg_open(const uint8_t* bytes, size_t n, JpegFile& jf) {
    jf.bytes = bytes;
    jf.n = n;
    jf.huff.resize(8);
    std::string err;
    const int rc = jpg::parse_headers(bytes, n, jf.fr, jf.huff.data(), &jf.scan_start, &err);
    return rc != jpg::kOk ? jpeg_fail(rc, err) : HPMVS_OK;
}

int jpeg_decode_scan(JpegFile& jf, int entropy, bool strict, uint32_t subseq_bits, float* ms) {
    const bool on_device = entropy == HPMVS_JPEG_ENTROPY_DEVICE ||
                           (entropy == HPMVS_JPEG_ENTROPY_AUTO && jf.n - jf.scan_start >= (size_t)HPMVS_JPEG_AUTO_MIN_SCAN_BYTES);
    if (on_device) {
        std::string why;
        const int rc = jpeg_entropy_device(jf, subseq_bits, &why, ms);
        if (rc != HPMVS_OK) return rc;
        if (why.empty()) {
            t_jpeg_last_used = jf.used;
            t_jpeg_last_rounds = jf.rounds;
            return HPMVS_OK;
        }
        if (strict) return fail(HPMVS_ERR_STATE, why);
    }
    std::string err;
    const int rc = jpg::decode_scan(jf.bytes, jf.n, jf.scan_start, jf.fr, jf.huff.data(), true, &err);
    if (rc != jpg::kOk) return jpeg_fail(rc, err);
    jf.used = HPMVS_JPEG_ENTROPY_HOST;
    jf.rounds = 0;
    t_jpeg_last_used = jf.used;
    t_jpeg_last_rounds = 0;
    return HPMVS_OK;
}

// Coefficients of a decoded frame -> interleaved RGB at the device address d_rgb (3 W H bytes), on the null stream of the
// current device; returns after the kernels have run.  The two working buffers (quantiser tables + coefficients, 2 bytes
// per sample; sample planes, 1 byte per sample) live for this call only: nothing is held between calls, so concurrent
// calls share nothing and a many-view upload accumulates nothing.
// ms (diagnostics, nullable): [1] coefficient upload, [2] IDCT kernel, [3] RGB kernel, from HIP events.
int jpeg_frame_to_device(const JpegFile& jf, uint8_t* d_rgb, float* ms) {
    const jpg::Frame& fr = jf.fr;
    jpg::Planes P;
    const size_t plane_bytes = jpg::make_planes(fr, &P);
    const size_t q_bytes = kJpegQBytes, coef_bytes = fr.n_blocks * 64 * sizeof(int16_t);
    uint16_t q[3 * 64] = {};
    for (int c = 0; c < fr.ncomp; c++) memcpy(q + 64 * c, fr.q[c], sizeof(uint16_t) * 64);
    DeviceBuffer d_own, d_planes;  // (d_own: the coefficient buffer when the host decoded the scan)
    if (!jf.d_coef) HIPCHK(d_own.alloc(q_bytes + coef_bytes));
    uint8_t* const d_coef = jf.d_coef ? jf.d_coef.p : d_own.p;
    HIPCHK(d_planes.alloc(plane_bytes));
    EventMarks ev(4, ms != nullptr);
    HIPCHK(ev.created());
    HIPCHK(ev.mark(0));
    HIPCHK(hipMemcpy(d_coef, q, q_bytes, hipMemcpyHostToDevice));
    if (!jf.d_coef) HIPCHK(hipMemcpy(d_coef + q_bytes, fr.coef.data(), coef_bytes, hipMemcpyHostToDevice));
    JpegBlocks B;
    B.n_blocks = (uint32_t)fr.n_blocks;
    B.first1 = fr.ncomp == 3 ? (uint32_t)(fr.c[1].off / 64) : B.n_blocks;
    B.first2 = fr.ncomp == 3 ? (uint32_t)(fr.c[2].off / 64) : B.n_blocks;
    B.bx0 = fr.c[0].bx;
    B.bx12 = fr.ncomp == 3 ? fr.c[1].bx : fr.c[0].bx;
    HIPCHK(ev.mark(1));
    launch_jpeg_idct((const uint16_t*)d_coef, (const int16_t*)(d_coef + q_bytes), B, P, d_planes.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(2));
    launch_jpeg_rgb(d_planes.p, P, d_rgb, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(3));
    HIPCHK(hipDeviceSynchronize());
    if (ms)
        for (int k = 0; k < 3; k++) HIPCHK(ev.elapsed(k, k + 1, &ms[1 + k]));
    return HPMVS_OK;
}

// ---- baseline JPEG encode (jpeg_enc.hpp, kernel_jpeg_encode.hip): everything between the pixels and the stuffed entropy data
// runs on the device; the host puts the header in front and EOI behind
// d_rgb: interleaved u8 [H][W][3] on the current device -> the whole file at the host address `out`, on the null stream.  *n is
// the file's length, also when cap is too small (HPMVS_ERR_ARG; nothing is written to `out` then).  The two working buffers
// live for this call only.  The first is sized from the image: tables, coefficients, the blocks' lengths and offsets.  The
// second is sized from the stream's length once the scan has given it, which jpeg_enc.hpp's bound (208 bytes per block,
// every byte stuffed) limits: the stream, its chunks' counts and offsets, and the stuffed bytes at twice the stream's length.
// ms (diagnostics, nullable): by HIP events [0] the first buffer and the tables' upload, [1] coefficient kernel, [2] lengths and their scan
// with the total's read-back, [3] the second buffer and its fills, [4] write kernel, [5] 0xFF counts and their scan with the
// total's read-back, [6] stuff kernel, [7] the bytes' copy to the host.
int jpeg_encode_device(const uint8_t* d_rgb, int W, int H, int quality, uint8_t* out, size_t cap, size_t* n, float* ms) {
    const jpge::Geom g = jpge::make_geom(W, H);
    jpge::EncTables T;
    jpge::make_tables(quality, &T);
    const size_t nb = g.n_blocks;
    DeviceBuffer work, work2;
    EventMarks ev(9, ms != nullptr);
    HIPCHK(ev.created());
    size_t scan_bytes = 0;
    HIPCHK((hipError_t)jpeg_enc_scan(nullptr, &scan_bytes, nullptr, nullptr, nb + 1, nullptr));
    Layout L;
    const size_t o_tabs = L.take(sizeof(T)), o_coef = L.take(nb * 64 * sizeof(int16_t)), o_lens = L.take((nb + 1) * 8), o_offs = L.take((nb + 1) * 8),
                 o_temp = L.take(scan_bytes);
    HIPCHK(ev.mark(0));
    HIPCHK(work.alloc(L.total));
    const jpge::EncTables* d_tabs = (const jpge::EncTables*)(work.p + o_tabs);
    int16_t* d_coef = (int16_t*)(work.p + o_coef);
    unsigned long long *d_lens = (unsigned long long*)(work.p + o_lens), *d_offs = (unsigned long long*)(work.p + o_offs);
    HIPCHK(hipMemcpy(work.p + o_tabs, &T, sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(d_lens + nb, 0, 8, nullptr));
    HIPCHK(ev.mark(1));
    launch_jpeg_enc_coef(d_rgb, g, d_tabs, d_coef, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(2));
    launch_jpeg_enc_lengths(d_coef, g.n_blocks, d_tabs, d_lens, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK((hipError_t)jpeg_enc_scan(work.p + o_temp, &scan_bytes, d_lens, d_offs, nb + 1, nullptr));
    unsigned long long bits = 0;
    HIPCHK(hipMemcpy(&bits, d_offs + nb, 8, hipMemcpyDeviceToHost));
    HIPCHK(ev.mark(3));
    if (bits == 0 || bits > (unsigned long long)nb * jpge::kBlockBoundBytes * 8) return fail(HPMVS_ERR_HIP, "jpeg_encode: the blocks' lengths are none the encoder produces");
    const unsigned long long n_bytes = (bits + 7) / 8, n_chunks = (n_bytes + 63) / 64;
    size_t scan2_bytes = 0;
    HIPCHK((hipError_t)jpeg_enc_scan(nullptr, &scan2_bytes, nullptr, nullptr, (size_t)n_chunks + 1, nullptr));
    Layout L2;
    const size_t o_stream = L2.take((size_t)n_chunks * 64), o_cnt = L2.take(((size_t)n_chunks + 1) * 8), o_moved = L2.take(((size_t)n_chunks + 1) * 8),
                 o_temp2 = L2.take(scan2_bytes), o_out = L2.take((size_t)n_bytes * 2);
    HIPCHK(work2.alloc(L2.total));
    unsigned long long *d_cnt = (unsigned long long*)(work2.p + o_cnt), *d_moved = (unsigned long long*)(work2.p + o_moved);
    HIPCHK(hipMemsetAsync(work2.p + o_stream, 0, (size_t)n_chunks * 64, nullptr));
    HIPCHK(hipMemsetAsync(d_cnt + n_chunks, 0, 8, nullptr));
    HIPCHK(ev.mark(4));
    launch_jpeg_enc_write(d_coef, g.n_blocks, d_tabs, d_offs, (uint32_t*)(work2.p + o_stream), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(5));
    launch_jpeg_enc_ff(work2.p + o_stream, n_chunks, d_cnt, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK((hipError_t)jpeg_enc_scan(work2.p + o_temp2, &scan2_bytes, d_cnt, d_moved, (size_t)n_chunks + 1, nullptr));
    unsigned long long n_ff = 0;
    HIPCHK(hipMemcpy(&n_ff, d_moved + n_chunks, 8, hipMemcpyDeviceToHost));
    HIPCHK(ev.mark(6));
    if (n_ff > n_bytes) return fail(HPMVS_ERR_HIP, "jpeg_encode: more stuffed bytes than bytes");
    const size_t n_data = (size_t)(n_bytes + n_ff);
    *n = jpge::kHeaderBytes + n_data + 2;
    if (cap < *n) return fail(HPMVS_ERR_ARG, "jpeg_encode: output buffer too small (" + std::to_string(*n) + " bytes needed)");
    launch_jpeg_enc_stuff(work2.p + o_stream, n_chunks, n_bytes, d_moved, work2.p + o_out, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(7));
    HIPCHK(hipMemcpy(out + jpge::kHeaderBytes, work2.p + o_out, n_data, hipMemcpyDeviceToHost));
    HIPCHK(ev.mark(8));
    jpge::write_header(W, H, quality, out);
    out[jpge::kHeaderBytes + n_data] = 0xFF;
    out[jpge::kHeaderBytes + n_data + 1] = 0xD9;
    if (ms) {
        HIPCHK(ev.sync(8));
        for (int k = 0; k < 8; k++) HIPCHK(ev.elapsed(k, k + 1, &ms[k]));
    }
    return HPMVS_OK;
}

}  // namespace capi
}  // namespace hpmvs

// an argument error found behind the header parse: the file's own refusal, if the scan has one, still comes first
static int jpeg_arg_error(JpegFile& jf, int code, const std::string& msg) {
    std::string err;
    const int rc = jpg::decode_scan(jf.bytes, jf.n, jf.scan_start, jf.fr, jf.huff.data(), false, &err);
    return rc != jpg::kOk ? jpeg_fail(rc, err) : fail(code, msg);
}

// strict: the caller asked for the device itself (jpeg_decode_scan)
static int jpeg_decode_impl(int device, const uint8_t* bytes, size_t n, uint8_t* rgb, size_t cap, int rgb_on_device, int entropy, bool strict,
                            int* used) {
    if (!bytes || !rgb) return fail(HPMVS_ERR_ARG, "jpeg_decode: null argument");
    if (!jpeg_entropy_ok(entropy)) return fail(HPMVS_ERR_ARG, "jpeg_decode: bad entropy value");
    JpegFile jf;
    if (const int rc = jpeg_open(bytes, n, jf)) return rc;
    const size_t nb = (size_t)3 * jf.fr.W * jf.fr.H;
    if (cap < nb) return jpeg_arg_error(jf, HPMVS_ERR_ARG, "jpeg_decode: output buffer smaller than 3 * width * height");
    // (a missing device and a bad index are argument errors too; only a device that cannot be made current is reported at once)
    if (const int rc = use_device(device, "jpeg_decode")) return rc == HPMVS_ERR_HIP ? rc : jpeg_arg_error(jf, rc, std::string(g_err));
    if (const int rc = jpeg_decode_scan(jf, entropy, strict)) return rc;
    if (used) *used = jf.used;
    if (rgb_on_device) return jpeg_frame_to_device(jf, rgb);
    DeviceBuffer d_rgb;
    HIPCHK(d_rgb.alloc(nb));
    if (const int rc = jpeg_frame_to_device(jf, d_rgb.p)) return rc;
    HIPCHK(hipMemcpy(rgb, d_rgb.p, nb, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

extern "C" {

int hpmvs_jpeg_info(const uint8_t* bytes, size_t n, int* width, int* height, int* components, int* h_samp, int* v_samp) {
    if (!bytes || !width || !height || !components || !h_samp || !v_samp) return fail(HPMVS_ERR_ARG, "jpeg_info: null argument");
    jpg::Frame fr;
    std::string err;
    const int rc = jpg::decode_file(bytes, n, fr, false, &err);
    if (rc != jpg::kOk) return jpeg_fail(rc, err);
    *width = fr.W; *height = fr.H; *components = fr.ncomp; *h_samp = fr.hmax; *v_samp = fr.vmax;
    return HPMVS_OK;
}

int hpmvs_jpeg_decode_ex(int device, const uint8_t* bytes, size_t n, uint8_t* rgb, size_t cap, int rgb_on_device, int entropy, int* used) {
    return jpeg_decode_impl(device, bytes, n, rgb, cap, rgb_on_device, entropy, entropy == HPMVS_JPEG_ENTROPY_DEVICE, used);
}

// (the environment's choice; its `device` is no request for the device itself and leaves to the host walk what _AUTO would)
int hpmvs_jpeg_decode(int device, const uint8_t* bytes, size_t n, uint8_t* rgb, size_t cap, int rgb_on_device) {
    return jpeg_decode_impl(device, bytes, n, rgb, cap, rgb_on_device, jpeg_entropy_env(), false, nullptr);
}

int hpmvs_jpeg_coefficients(int device, const uint8_t* bytes, size_t n, int entropy, int subseq_bits, int16_t* coef, size_t cap, int* used,
                            int* rounds) {
    if (!bytes || !coef) return fail(HPMVS_ERR_ARG, "jpeg_coefficients: null argument");
    if (!jpeg_entropy_ok(entropy)) return fail(HPMVS_ERR_ARG, "jpeg_coefficients: bad entropy value");
    if (subseq_bits != 0 && (subseq_bits < 64 || subseq_bits % 32 != 0))
        return fail(HPMVS_ERR_ARG, "jpeg_coefficients: subseq_bits must be 0 or a multiple of 32 from 64 up");
    JpegFile jf;
    if (const int rc = jpeg_open(bytes, n, jf)) return rc;
    const size_t nc = jf.fr.n_blocks * 64;
    if (cap < nc) return fail(HPMVS_ERR_ARG, "jpeg_coefficients: output buffer smaller than the frame's coefficients");
    if (const int rc = use_device(device, "jpeg_coefficients")) return rc;
    if (const int rc = jpeg_decode_scan(jf, entropy, entropy == HPMVS_JPEG_ENTROPY_DEVICE,
                                        subseq_bits ? (uint32_t)subseq_bits : (uint32_t)jpg::kSubseqBits))
        return rc;
    if (jf.d_coef) HIPCHK(hipMemcpy(coef, jf.d_coef.p + kJpegQBytes, nc * sizeof(int16_t), hipMemcpyDeviceToHost));
    else memcpy(coef, jf.fr.coef.data(), nc * sizeof(int16_t));
    if (used) *used = jf.used;
    if (rounds) *rounds = jf.rounds;
    return HPMVS_OK;
}

int hpmvs_jpeg_last_decode(int* used, int* rounds) {
    if (!used) return fail(HPMVS_ERR_ARG, "jpeg_last_decode: null argument");
    if (t_jpeg_last_used < 0) return fail(HPMVS_ERR_STATE, "jpeg_last_decode: this thread has decoded no JPEG scan yet");
    *used = t_jpeg_last_used;
    if (rounds) *rounds = t_jpeg_last_rounds;
    return HPMVS_OK;
}

int hpmvs_jpeg_decode_timed(int device, const uint8_t* bytes, size_t n, uint8_t* rgb_device, size_t cap, float* ms) {
    if (!bytes || !rgb_device || !ms) return fail(HPMVS_ERR_ARG, "jpeg_decode_timed: null argument");
    JpegFile jf;  // (the host walks the whole file here, under the clock: no jpeg_open, no device buffer)
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = jpg::decode_file(bytes, n, jf.fr, true, &err);
    ms[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != jpg::kOk) return jpeg_fail(rc, err);
    if (cap < (size_t)3 * jf.fr.W * jf.fr.H) return fail(HPMVS_ERR_ARG, "jpeg_decode_timed: output buffer smaller than 3 * width * height");
    if (const int rd = use_device(device, "jpeg_decode_timed")) return rd;
    return jpeg_frame_to_device(jf, rgb_device, ms);
}

int hpmvs_jpeg_entropy_timed(int device, const uint8_t* bytes, size_t n, uint8_t* rgb_device, size_t cap, float* ms) {
    if (!bytes || !rgb_device || !ms) return fail(HPMVS_ERR_ARG, "jpeg_entropy_timed: null argument");
    JpegFile jf;
    if (const int rc = jpeg_open(bytes, n, jf)) return rc;
    if (cap < (size_t)3 * jf.fr.W * jf.fr.H) return fail(HPMVS_ERR_ARG, "jpeg_entropy_timed: output buffer smaller than 3 * width * height");
    if (const int rc = use_device(device, "jpeg_entropy_timed")) return rc;
    for (int k = 0; k < 12; k++) ms[k] = 0.0f;
    if (const int rc = jpeg_decode_scan(jf, HPMVS_JPEG_ENTROPY_DEVICE, true, jpg::kSubseqBits, ms)) return rc;
    ms[11] = (float)jf.rounds;
    return jpeg_frame_to_device(jf, rgb_device, ms + 7);
}

size_t hpmvs_jpeg_encode_bound(int width, int height) {
    if (width < 1 || height < 1 || width > jpge::kMaxSide || height > jpge::kMaxSide) return 0;
    return jpge::encode_bound(width, height);
}

static int jpeg_encode_impl(int device, const uint8_t* rgb, int width, int height, int quality, uint8_t* out, size_t cap, size_t* n,
                            int rgb_on_device, float* ms) {
    if (!rgb || !out || !n) return fail(HPMVS_ERR_ARG, "jpeg_encode: null argument");
    std::string err;
    const int rc = jpge::check_args(width, height, quality, &err);
    if (rc != jpge::kOk) return jpeg_enc_fail(rc, err);
    if (const int rd = use_device(device, "jpeg_encode")) return rd;
    if (rgb_on_device) return jpeg_encode_device(rgb, width, height, quality, out, cap, n, ms);
    const size_t nb = (size_t)3 * width * height;
    DeviceBuffer d_rgb;
    HIPCHK(d_rgb.alloc(nb));
    HIPCHK(hipMemcpy(d_rgb.p, rgb, nb, hipMemcpyHostToDevice));
    return jpeg_encode_device(d_rgb.p, width, height, quality, out, cap, n, ms);
}

int hpmvs_jpeg_encode(int device, const uint8_t* rgb, int width, int height, int quality, uint8_t* out, size_t cap, size_t* n, int rgb_on_device) {
    return jpeg_encode_impl(device, rgb, width, height, quality, out, cap, n, rgb_on_device, nullptr);
}

int hpmvs_jpeg_encode_timed(int device, const uint8_t* rgb_device, int width, int height, int quality, uint8_t* out, size_t cap, size_t* n, float* ms) {
    if (!ms) return fail(HPMVS_ERR_ARG, "jpeg_encode_timed: null argument");
    return jpeg_encode_impl(device, rgb_device, width, height, quality, out, cap, n, 1, ms);
}

// ---- the pyramid step and the radial undistortion on their own (kernels_basic.hip, kernel_undistort.hip)
int hpmvs_build_pyramid(int device, const uint8_t* src, int w, int h, uint8_t* dst, int on_device) {
    if (!src || !dst || w < 2 || h < 2) return fail(HPMVS_ERR_ARG, "build_pyramid: bad argument");
    if (const int rc = use_device(device, "build_pyramid")) return rc;
    const size_t nb = (size_t)w * h * 3, nb2 = (size_t)(w / 2) * (h / 2) * 3;
    if (on_device) {
        launch_half_resize(src, w, h, dst, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        return HPMVS_OK;
    }
    DeviceBuffer ds, dd;
    HIPCHK(ds.alloc(nb));
    HIPCHK(dd.alloc(nb2 + 16));
    HIPCHK(hipMemcpy(ds.p, src, nb, hipMemcpyHostToDevice));
    launch_half_resize(ds.p, w, h, dd.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(dst, dd.p, nb2, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

int hpmvs_undistort(int device, const uint8_t* src, int w, int h, float f, float k1, uint8_t* dst, int on_device) {
    if (!src || !dst || w < 2 || h < 2) return fail(HPMVS_ERR_ARG, "undistort: bad argument");
    if (!undistort_args_ok(f, k1)) return fail(HPMVS_ERR_ARG, "undistort: f must be finite and > 0, k1 finite");
    const size_t nb = (size_t)w * h * 3;
    if (src < dst + nb && dst < src + nb) return fail(HPMVS_ERR_ARG, "undistort: src and dst overlap");
    if (const int rc = use_device(device, "undistort")) return rc;
    if (k1 == 0.0f) {  // Image::load undistorts only for k1 != 0 (reference Image.cpp:50-53)
        HIPCHK(hipMemcpy(dst, src, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost));
        return HPMVS_OK;
    }
    if (on_device) {
        launch_undistort(src, w, h, f, k1, dst, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        return HPMVS_OK;
    }
    DeviceBuffer ds, dd;
    HIPCHK(ds.alloc(nb));
    HIPCHK(dd.alloc(nb));
    HIPCHK(hipMemcpy(ds.p, src, nb, hipMemcpyHostToDevice));
    launch_undistort(ds.p, w, h, f, k1, dd.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(dst, dd.p, nb, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

int hpmvs_undistort_map(int device, int w, int h, float f, float k1, float* xy) {
    if (!xy || w < 2 || h < 2) return fail(HPMVS_ERR_ARG, "undistort_map: bad argument");
    if (!undistort_args_ok(f, k1)) return fail(HPMVS_ERR_ARG, "undistort_map: f must be finite and > 0, k1 finite");
    if (const int rc = use_device(device, "undistort_map")) return rc;
    const size_t nf = (size_t)w * h * 2;
    DeviceBuffer dxy;
    HIPCHK(dxy.alloc(nf * sizeof(float)));
    launch_undistort_map(w, h, f, k1, (float*)dxy.p, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(xy, dxy.p, nf * sizeof(float), hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

}  // extern "C"

// ---- depth maps as jet-coloured images (depth_vis.hpp, kernel_depth_vis.hip; reference Scene::visualizeDepths)
// the image of `level` (or HPMVS_DEPTH_COMBINED): cols x rows of that level, of level 0 for the combined one
static void depth_image_size(const SceneDepthMaps& dm, int level, int* W, int* H) {
    const int l = level == HPMVS_DEPTH_COMBINED ? 0 : level;
    *W = dm.maps.cols[l];
    *H = dm.maps.rows[l];
}

// The image at the device address d_rgb (3 W H bytes) on the scene's device, which the caller made current; W, H > 0.  Ordered
// behind pending map writes as hpmvs_scene_depth_get_level is: the null stream is drained first and the kernels run on it.
// Returns after they have run.  The working buffer (the float image, the workgroups' minima and maxima, the colormap, m and
// M) lives for this call only, so concurrent calls share nothing.  The maps are read, never written.
static int depth_image_device(const SceneDepthMaps& dm, int level, int W, int H, uint8_t* d_rgb, float range[2]) {
    const size_t n = (size_t)W * H;
    const unsigned n_part = depth_vis_partials(W, H);
    uint8_t lut[768];
    dvis::make_colormap(lut);
    Layout L;
    const size_t o_vals = L.take(n * sizeof(float)), o_part = L.take((size_t)2 * n_part * sizeof(float)), o_lut = L.take(sizeof(lut)),
                 o_range = L.take(2 * sizeof(float));
    DeviceBuffer work;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(work.alloc(L.total));
    HIPCHK(hipMemcpy(work.p + o_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
    launch_depth_vis_gather(dm.maps, dm.n_levels, level == HPMVS_DEPTH_COMBINED ? -1 : level, W, H, (float*)(work.p + o_vals),
                            (float*)(work.p + o_part), nullptr);
    HIPCHK(hipGetLastError());
    launch_depth_vis_colour((const float*)(work.p + o_vals), n, (const float*)(work.p + o_part), n_part, work.p + o_lut, d_rgb,
                            (float*)(work.p + o_range), nullptr);
    HIPCHK(hipGetLastError());
    float mM[2] = {0.0f, 0.0f};
    HIPCHK(hipMemcpy(mM, work.p + o_range, sizeof(mM), hipMemcpyDeviceToHost));  // (waits for both kernels)
    if (range) { range[0] = mM[0]; range[1] = mM[1]; }
    return HPMVS_OK;
}

extern "C" {

int hpmvs_depth_colormap(uint8_t lut[768]) {
    if (!lut) return fail(HPMVS_ERR_ARG, "depth_colormap: null argument");
    dvis::make_colormap(lut);
    return HPMVS_OK;
}

int hpmvs_scene_depth_image(const hpmvs_scene* s, int view, int level, uint8_t* rgb, size_t cap, int rgb_on_device, int* width, int* height,
                            float range[2]) {
    SceneDepthMaps dm;
    if (const int rc = scene_depth_maps(s, view, level, "scene_depth_image", &dm)) return rc;
    int W, H;
    depth_image_size(dm, level, &W, &H);
    if (width) *width = W;
    if (height) *height = H;
    if (!rgb) return HPMVS_OK;  // size query
    const size_t nb = (size_t)3 * W * H;
    if (cap < nb) return fail(HPMVS_ERR_ARG, "scene_depth_image: buffer smaller than 3 * width * height");
    if (nb == 0) {  // (a level of one pixel has a map without rows)
        if (range) range[0] = range[1] = 0.0f;
        return HPMVS_OK;
    }
    HIPCHK(hipSetDevice(dm.device));
    if (rgb_on_device) return depth_image_device(dm, level, W, H, rgb, range);
    DeviceBuffer d_rgb;
    HIPCHK(d_rgb.alloc(nb));
    if (const int rc = depth_image_device(dm, level, W, H, d_rgb.p, range)) return rc;
    HIPCHK(hipMemcpy(rgb, d_rgb.p, nb, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

int hpmvs_scene_depth_jpeg(const hpmvs_scene* s, int view, int level, int quality, uint8_t* out, size_t cap, size_t* n) {
    if (!n) return fail(HPMVS_ERR_ARG, "scene_depth_jpeg: null argument");
    SceneDepthMaps dm;
    if (const int rc = scene_depth_maps(s, view, level, "scene_depth_jpeg", &dm)) return rc;
    int W, H;
    depth_image_size(dm, level, &W, &H);
    std::string err;
    const int rc = jpge::check_args(W, H, quality, &err);
    if (rc != jpge::kOk) return jpeg_enc_fail(rc, err);
    if (!out) {
        *n = jpge::encode_bound(W, H);
        return HPMVS_OK;
    }
    HIPCHK(hipSetDevice(dm.device));
    DeviceBuffer d_rgb;
    HIPCHK(d_rgb.alloc((size_t)3 * W * H));
    if (const int rd = depth_image_device(dm, level, W, H, d_rgb.p, nullptr)) return rd;
    return jpeg_encode_device(d_rgb.p, W, H, quality, out, cap, n);
}

}  // extern "C"
