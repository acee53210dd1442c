// capi.hip -- the C ABI of include/hpmvs_amd.h: scene residency in HBM + batch launches (the image entry points, which
// touch no scene, are capi_image.hip's).  Host-side only; all arithmetic of the hot path is in the kernels.  There is
// no CPU fallback: without a HIP device every compute entry point fails with HPMVS_ERR_NODEVICE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <time.h>
#include <vector>

#include "../../include/hpmvs_amd.h"
#include "capi_common.hpp"
#include "dev_types.h"
#include "launch.h"
#include "octree.hpp"
#include "ply_text.hpp"

using namespace hpmvs;
using namespace hpmvs::capi;

// Each optimize launch gets its own workspace (work-queue counter block + the per-slot image-list rows),
// handed out round-robin, so that launches issued concurrently from several host threads / streams (the
// reference runs one PatchOptimizer per OpenMP thread against one shared Scene: src/hpmvs/Scene.cpp:94-96,
// 166-167) never share one.  16 launches in flight per scene; each of them fills the GPU.
static constexpr int kQueueSlots = 16;
static constexpr size_t kQueueSlotBytes = 1024;
static constexpr int kServiceMaxPatches = 4;  // host batches up to this size go through the open batch (Service)  // the counter block at the head of a workspace (zeroed per launch)

thread_local std::string hpmvs::capi::g_err;

struct hpmvs_scene {
    int device = 0;
    int n_views = 0;
    int n_cus = 256;
    bool committed = false;
    std::vector<DevView> hviews;
    std::vector<char> view_set;
    std::vector<std::vector<int32_t>> covis;
    std::vector<void*> allocs;
    DevView* dviews = nullptr;
    int32_t* dcovis_off = nullptr;
    int32_t* dcovis = nullptr;
    // open batches behind single-patch host calls (see Service below); two, so that one can drain while the other is open
    struct Service;
    mutable Service* svc[2] = {nullptr, nullptr};
    mutable int svc_cur = 0;
    mutable std::mutex svc_mu;
    // depth maps (hpmvs_scene_depth_reset): one pool, per view a table of level pointers
    mutable float* depth_pool = nullptr;
    mutable size_t depth_floats = 0;
    mutable DevDepthView* ddepth = nullptr;
    mutable std::vector<DevDepthView> hdepth;
    mutable int32_t* dqueue[kQueueSlots] = {};  // launch workspaces of ws_bytes each: the first at commit, the others on first concurrent use
    mutable int n_queues = 0;
    size_t ws_bytes = 0;
    mutable unsigned next_slot = 0;
    mutable int32_t* last_queue = nullptr;
    mutable std::atomic<unsigned long long> last_staged_bytes{0}, last_mapped_bytes{0};  // of the last host-pointer optimize_batch call
    size_t bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t slot_done[kQueueSlots] = {};   // recorded behind the last launch that used workspace k
    mutable bool slot_used[kQueueSlots] = {};
    mutable hipStream_t slot_stream[kQueueSlots] = {};   // the stream workspace k's last launch went to
    mutable std::recursive_mutex mu;  // (recursive: Exclusive scopes nest with the workspace hand-out)
    mutable bool timed = false;
    // Small host-pointer batches (the unchanged callers' optimize() = batch of 1, and what a combiner makes of
    // concurrent callers) are staged through persistent blocks: pinned host + device memory and a stream per
    // entry, one H2D and one D2H copy per call, no hipMalloc / hipFree
    struct StageEntry { hipStream_t st = nullptr; char* dev = nullptr; char* host = nullptr; std::mutex mu; };
    static constexpr int kStageEntries = 8;
    mutable int32_t* last_ws = nullptr;   // the workspace of the last refinement launch (hpmvs_last_wide_patches)
    mutable std::atomic<int32_t> last_walk[3] = {};   // hpmvs_last_level_walk: rounds, most rounds in a wave, in-order passes
    static constexpr int kStageCapPatches = 4096;
    mutable StageEntry stage[kStageEntries];
    mutable std::atomic<unsigned> stage_next{0};
};

static int service_quiesce(const hpmvs_scene* s);
static void service_close_all(const hpmvs_scene* s);
static void service_free(hpmvs_scene* s);

// Workspace hand-out (call with s->mu held).  Before a workspace is reused the launch that used it last must
// have finished: more than kQueueSlots launches in flight against one scene (e.g. 256 OpenMP threads each
// calling optimize()) simply queue up here instead of sharing a counter / image-list rows.
static int acquire_workspace(const hpmvs_scene* s, int32_t** q, int* slot, hipStream_t st) {
    // The workspace whose last launch went to THIS stream is taken again without any wait: the counter-block memset and the
    // kernel of the new launch are ordered behind the old one by the stream itself (a scheduler that enqueues round after
    // round on one stream, like bench.py, never needs a second workspace).  Otherwise one whose last launch has finished;
    // only when every allocated one is still in flight on OTHER streams does the scene grow another (~210 MB each), and
    // with all kQueueSlots in flight the caller waits for the oldest.
    int k = -1;
    for (int i = 0; i < s->n_queues && k < 0; i++)
        if (s->slot_used[i] && s->slot_stream[i] == st) k = i;
    for (int i = 0; i < s->n_queues && k < 0; i++) {
        const int c = (int)((s->next_slot + i) % (unsigned)s->n_queues);
        if (!s->slot_used[c]) k = c;
        else if (hipEventQuery(s->slot_done[c]) == hipSuccess) k = c;
        else (void)hipGetLastError();  // hipErrorNotReady is not an error here
    }
    if (k < 0 && s->n_queues < kQueueSlots) {
        int32_t* w = nullptr;
        HIPCHK(hipMalloc((void**)&w, s->ws_bytes));
        // cleared ON THE LAUNCH STREAM: hipMemset on the null stream returns before the fill has run and is not ordered with the
        // non-blocking streams small host batches are launched on -- the fill of a workspace that was grown under concurrent
        // single-patch calls ran INTO the first launch that used it and zeroed its image-list rows (round 6: one call in a few
        // hundred came back with another refinement; tests/test_gpu_concurrent_first_calls.py)
        if (hipMemsetAsync(w, 0, s->ws_bytes, st) != hipSuccess) { hipFree(w); return fail(HPMVS_ERR_HIP, "cannot clear a launch workspace"); }
        k = s->n_queues;
        s->dqueue[k] = w;
        s->n_queues++;
        const_cast<hpmvs_scene*>(s)->bytes += s->ws_bytes;
    }
    if (k < 0) {
        k = (int)(s->next_slot % kQueueSlots);
        HIPCHK(hipEventSynchronize(s->slot_done[k]));
    }
    // whatever path chose it: the new launch is ordered behind the workspace's previous one on the device (a no-op for the
    // same stream and for a finished launch; it also covers a stream handle that was destroyed and handed out again)
    if (s->slot_used[k]) HIPCHK(hipStreamWaitEvent(st, s->slot_done[k], 0));
    s->next_slot = (unsigned)k + 1;
    s->slot_stream[k] = st;
    *q = s->dqueue[k];
    *slot = k;
    s->last_queue = *q;
    return HPMVS_OK;
}
// A workspace (q) for the work a call enqueues on `st`: declare it with s->mu held, and check rc.  Whatever happens behind the
// declaration, the slot's event is recorded behind the work that was enqueued, so that the next user of the workspace waits for it.
struct Workspace {
    const hpmvs_scene* s;
    hipStream_t st;
    int32_t* q = nullptr;
    int slot = 0, rc;
    Workspace(const hpmvs_scene* s_, hipStream_t st_) : s(s_), st(st_) { rc = acquire_workspace(s, &q, &slot, st); }
    ~Workspace() { if (!rc) { hipEventRecord(s->slot_done[slot], st); s->slot_used[slot] = true; } }
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
};

extern "C" {

const char* hpmvs_last_error(void) { return g_err.c_str(); }
#ifndef HPMVS_BUILD_ID
#define HPMVS_BUILD_ID "unstamped"
#endif
const char* hpmvs_build_id(void) { return HPMVS_BUILD_ID; }

int hpmvs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void hpmvs_default_options(hpmvs_options* o) {
    // reference include/hpmvs/HpmvsOptions.h:29-58
    o->MAXLEVEL = 5;
    o->MINLEVEL = 0;
    o->MAX_ANGLE = (float)(60.0f * M_PI / 180.0f);
    o->MIN_ANGLE = (float)(10.0f * M_PI / 180.0f);
    o->MAX_IMAGES_PER_PATCH = 6;
    o->MIN_IMAGES_PER_PATCH = 3;
    o->NCC_ALPHA_1 = 0.4f;
    o->NCC_ALPHA_2 = 0.5f;
}

static DevOptions make_dev_options(const hpmvs_options* o) {
    DevOptions d;
    d.MAXLEVEL = o->MAXLEVEL; d.MINLEVEL = o->MINLEVEL;
    d.MAX_ANGLE = o->MAX_ANGLE; d.MIN_ANGLE = o->MIN_ANGLE;
    d.MAX_IMAGES_PER_PATCH = o->MAX_IMAGES_PER_PATCH; d.MIN_IMAGES_PER_PATCH = o->MIN_IMAGES_PER_PATCH;
    d.NCC_ALPHA_1 = o->NCC_ALPHA_1; d.NCC_ALPHA_2 = o->NCC_ALPHA_2;
    d.cos_max_d = cos((double)o->MAX_ANGLE);
    d.cos_max_f = std::cos(o->MAX_ANGLE);
    d.sort_thr = (float)(1.0f - cos(10.0 * M_PI / 180.0));
    d.angle_scale = (float)(M_PI / 48.0f);
    return d;
}

// Camera::init, reference src/hpmvs/Camera.cpp:34-81 (float32 after the float64 quaternion)
int hpmvs_camera_from_nvm(double f, const double q[4], const double c[3], int width, int height, int max_level,
                          hpmvs_camera* out) {
    if (!q || !c || !out || width < 1 || height < 1 || max_level < 0 || max_level + 1 > HPMVS_MAX_LEVELS)
        return fail(HPMVS_ERR_ARG, "camera_from_nvm: bad argument");
    const float K[9] = {(float)f, 0.f, (float)(width / 2.0), 0.f, (float)f, (float)(height / 2.0), 0.f, 0.f, 1.f};
    // Eigen::Quaterniond::matrix() in double (Camera.cpp:43-50), no normalisation
    const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
    const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
    const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
    const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
    const float R[9] = {(float)(1.0 - (tyy + tzz)), (float)(txy - twz), (float)(txz + twy),
                        (float)(txy + twz), (float)(1.0 - (txx + tzz)), (float)(tyz - twx),
                        (float)(txz - twy), (float)(tyz + twx), (float)(1.0 - (txx + tyy))};
    const float cf[3] = {(float)c[0], (float)c[1], (float)c[2]};
    float Rt[12];
    for (int r = 0; r < 3; r++) {
        Rt[r * 4 + 0] = R[r * 3 + 0]; Rt[r * 4 + 1] = R[r * 3 + 1]; Rt[r * 4 + 2] = R[r * 3 + 2];
        Rt[r * 4 + 3] = -((R[r * 3 + 0] * cf[0] + R[r * 3 + 1] * cf[1]) + R[r * 3 + 2] * cf[2]);
    }
    for (int r = 0; r < 3; r++)
        for (int col = 0; col < 4; col++)
            out->P0[r * 4 + col] =
                (K[r * 3 + 0] * Rt[0 * 4 + col] + K[r * 3 + 1] * Rt[1 * 4 + col]) + K[r * 3 + 2] * Rt[2 * 4 + col];
    out->center[0] = cf[0]; out->center[1] = cf[1]; out->center[2] = cf[2]; out->center[3] = 1.0f;
    const float* r2 = &out->P0[8];
    const float nrm = std::sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]);
    float z[3] = {r2[0] / nrm, r2[1] / nrm, r2[2] / nrm};
    float x[3] = {out->P0[0], out->P0[1], out->P0[2]};
    auto cross = [](const float* a, const float* b, float* o) {
        const float o0 = a[1] * b[2] - a[2] * b[1], o1 = a[2] * b[0] - a[0] * b[2], o2 = a[0] * b[1] - a[1] * b[0];
        o[0] = o0; o[1] = o1; o[2] = o2;
    };
    auto normalize = [](float* a) {
        const float n2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        if (n2 > 0.f) { const float n = std::sqrt(n2); a[0] /= n; a[1] /= n; a[2] /= n; }
    };
    float y[3];
    cross(z, x, y); normalize(y);
    cross(y, z, x); normalize(x);
    for (int k = 0; k < 3; k++) { out->xaxis[k] = x[k]; out->yaxis[k] = y[k]; out->zaxis[k] = z[k]; }
    out->fsum = K[0] + K[4];
    out->n_levels = max_level + 1;
    return HPMVS_OK;
}

// Scene::getSceneCenter, reference src/hpmvs/Scene.cpp:210-239 over TriangulateMidpoint (include/hpmvs/Triangulation.hpp:28-53):
// the point closest to every camera's optical axis and the largest distance from it to a camera centre.  Float64, host only.
// The 4x4 system is accumulated with the reference's expressions in camera order; it is solved by Householder QR with
// column pivoting like the reference's Eigen::ColPivHouseholderQR, but not by Eigen's code: equal to solver accuracy.
int hpmvs_scene_center(const hpmvs_camera* cams, int n, double center[3], double* radius, int* valid) {
    if (!center || !radius || !valid || n < 0 || (n > 0 && !cams)) return fail(HPMVS_ERR_ARG, "scene_center: bad argument");
    *valid = 0;
    center[0] = center[1] = center[2] = 0.0;
    *radius = 0.0;
    if (n < 2) return HPMVS_OK;  // n == 0: the reference returns false (Scene.cpp:218); n == 1: its CHECK_GE(origins.size(), 2) aborts
    double A[4][4] = {{0}}, b[4] = {0};
    std::vector<double> org((size_t)3 * n);
    for (int i = 0; i < n; i++) {
        // cam.oAxis_.head<3>().cast<double>().normalized(), cam.center_.cast<double>().hnormalized() (Scene.cpp:215-216)
        const double z[3] = {(double)cams[i].zaxis[0], (double)cams[i].zaxis[1], (double)cams[i].zaxis[2]};
        const double nz = std::sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
        const double d[4] = {z[0] / nz, z[1] / nz, z[2] / nz, 0.0};
        const double w = (double)cams[i].center[3];
        double* o = &org[(size_t)3 * i];
        for (int k = 0; k < 3; k++) o[k] = (double)cams[i].center[k] / w;
        const double oh[4] = {o[0], o[1], o[2], 1.0};
        for (int r = 0; r < 4; r++) {
            double t[4];
            for (int c = 0; c < 4; c++) t[c] = (r == c ? 1.0 : 0.0) - d[r] * d[c];  // A_term = I - d_h d_h^T
            for (int c = 0; c < 4; c++) A[r][c] += t[c];
            b[r] += ((t[0] * oh[0] + t[1] * oh[1]) + t[2] * oh[2]) + t[3] * oh[3];
        }
    }
    // Householder QR with column pivoting: A P = Q R, applied to b as it goes
    int perm[4] = {0, 1, 2, 3};
    double rdiag0 = 0.0;
    for (int k = 0; k < 4; k++) {
        int piv = k;
        double best = -1.0;
        for (int c = k; c < 4; c++) {
            double s2 = 0.0;
            for (int r = k; r < 4; r++) s2 += A[r][c] * A[r][c];
            if (s2 > best) { best = s2; piv = c; }  // (NaN never wins: the solution is checked below)
        }
        if (piv != k) {
            for (int r = 0; r < 4; r++) std::swap(A[r][k], A[r][piv]);
            std::swap(perm[k], perm[piv]);
        }
        const double nrm = std::sqrt(best);
        if (k == 0) rdiag0 = nrm;
        // Numerically rank deficient: |R_kk| <= 64 * 2^-52 * |R_00|.  The fourth column of A is (0, 0, 0, n) and no column is
        // longer, so this is the 3x3 block sum(I - d d^T) having an eigenvalue below ~1.4e-14 n: axes parallel to ~1e-7 rad.
        if (!(nrm > 64.0 * 2.220446049250313e-16 * rdiag0)) return HPMVS_OK;
        const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
        double v[4] = {0, 0, 0, 0};
        v[k] = A[k][k] - alpha;
        for (int r = k + 1; r < 4; r++) v[r] = A[r][k];
        double vv = 0.0;
        for (int r = k; r < 4; r++) vv += v[r] * v[r];
        if (vv > 0.0) {
            for (int c = k; c < 4; c++) {
                double dot = 0.0;
                for (int r = k; r < 4; r++) dot += v[r] * A[r][c];
                const double f = 2.0 * dot / vv;
                for (int r = k; r < 4; r++) A[r][c] -= f * v[r];
            }
            double dot = 0.0;
            for (int r = k; r < 4; r++) dot += v[r] * b[r];
            const double f = 2.0 * dot / vv;
            for (int r = k; r < 4; r++) b[r] -= f * v[r];
        }
    }
    double y[4], x[4];
    for (int k = 3; k >= 0; k--) {
        double t = b[k];
        for (int c = k + 1; c < 4; c++) t -= A[k][c] * y[c];
        y[k] = t / A[k][k];
    }
    for (int k = 0; k < 4; k++) x[perm[k]] = y[k];
    const double ctr[3] = {x[0] / x[3], x[1] / x[3], x[2] / x[3]};  // center_homog.hnormalized() (Scene.cpp:225)
    double rmax = 0.0;  // radius = dists[dists.size() - 1] of the sorted distances: the maximum (Scene.cpp:233)
    for (int i = 0; i < n; i++) {
        const double e[3] = {ctr[0] - org[3 * i], ctr[1] - org[3 * i + 1], ctr[2] - org[3 * i + 2]};
        const double dist = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        if (!(dist <= rmax)) rmax = dist;  // (a NaN distance surfaces here and fails the check below)
    }
    if (!std::isfinite(ctr[0]) || !std::isfinite(ctr[1]) || !std::isfinite(ctr[2]) || !std::isfinite(rmax)) return HPMVS_OK;
    center[0] = ctr[0]; center[1] = ctr[1]; center[2] = ctr[2];
    *radius = rmax;
    *valid = 1;
    return HPMVS_OK;
}

int hpmvs_scene_create(int n_views, int device, hpmvs_scene** out) {
    if (!out || n_views <= 0 || n_views > 65535) return fail(HPMVS_ERR_ARG, "scene_create: bad n_views/out");
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (const int rc = use_device(device, "scene_create")) return rc;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    hpmvs_scene* s = new hpmvs_scene();
    struct Guard { hpmvs_scene* p; ~Guard() { if (p) { if (p->ev0) hipEventDestroy(p->ev0); if (p->ev1) hipEventDestroy(p->ev1); delete p; } } } guard{s};
    s->device = device;
    s->n_views = n_views;
    s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    s->hviews.resize(n_views);
    memset(s->hviews.data(), 0, sizeof(DevView) * (size_t)n_views);
    s->view_set.assign(n_views, 0);
    s->covis.resize(n_views);
    HIPCHK(hipEventCreate(&s->ev0));
    HIPCHK(hipEventCreate(&s->ev1));
    guard.p = nullptr;
    *out = s;
    return HPMVS_OK;
}

// hpmvs_scene_set_view and, for k1 != 0, hpmvs_scene_set_view_distorted: level 0 is the raw view undistorted on the GPU
// (jf: hpmvs_scene_set_view_jpeg_ex -- the raw level 0 is decoded on the device from the frame's coefficients; rgb_l0 is unused)
static int set_view(hpmvs_scene* s, int view, int width, int height, const uint8_t* rgb_l0, int rgb_on_device,
                    const hpmvs_camera* cam, float f, float k1, const JpegFile* jf = nullptr) {
    if (!s || !cam || (!rgb_l0 && !jf)) return fail(HPMVS_ERR_ARG, "scene_set_view: null argument");
    if (s->committed) return fail(HPMVS_ERR_STATE, "scene_set_view: scene already committed");
    if (view < 0 || view >= s->n_views || width < 2 || height < 2) return fail(HPMVS_ERR_ARG, "scene_set_view: bad view/size");
    if (cam->n_levels < 1 || cam->n_levels > HPMVS_MAX_LEVELS) return fail(HPMVS_ERR_ARG, "scene_set_view: bad n_levels");
    HIPCHK(hipSetDevice(s->device));
    DevView& V = s->hviews[view];
    // Image::init/load: max(1, MAXLEVEL) + 1 pyramid levels (reference Image.cpp:33-57); the camera has
    // MAXLEVEL + 1 projection levels (Camera.cpp:36).  Both are MAXLEVEL + 1 for MAXLEVEL >= 1.
    const int levels = cam->n_levels < 2 ? 2 : cam->n_levels;
    // one allocation per view: level l at a 256-byte aligned offset, 16 B of padding behind every level
    size_t off[HPMVS_MAX_LEVELS] = {}, total = 0;
    {
        int w = width, h = height;
        for (int l = 0; l < levels; l++) {
            if (w < 1 || h < 1) return fail(HPMVS_ERR_ARG, "scene_set_view: image too small for the pyramid depth");
            off[l] = total;
            total += ((size_t)w * h * 3 + 16 + 255) & ~(size_t)255;
            w /= 2; h /= 2;
        }
        if (total > 0xffffffffull) return fail(HPMVS_ERR_ARG, "scene_set_view: image too large (a view's pyramid must stay below 4 GB)");
    }
    // the raw view of a distorted one on the device: the caller's buffer, or a copy of the host pixels
    const uint8_t* raw = nullptr;
    DeviceBuffer raw_copy;
    if (k1 != 0.0f) {
        if (rgb_on_device && !jf) {
            raw = rgb_l0;
        } else {
            HIPCHK(raw_copy.alloc((size_t)width * height * 3));
            if (!jf) HIPCHK(hipMemcpy(raw_copy.p, rgb_l0, (size_t)width * height * 3, hipMemcpyHostToDevice));
            raw = raw_copy.p;
        }
    }
    uint8_t* slab = nullptr;
    HIPCHK(hipMalloc((void**)&slab, total));
    if (s->view_set[view]) {  // set again: release the previous pyramid of this view
        void* old = (void*)V.pix[0];
        for (size_t k = 0; k < s->allocs.size(); k++)
            if (s->allocs[k] == old) { s->allocs.erase(s->allocs.begin() + k); break; }
        if (old) { hipFree(old); s->bytes -= V.slab_bytes; }
        for (int l = 0; l < HPMVS_MAX_LEVELS; l++) V.pix[l] = nullptr;
        s->view_set[view] = 0;
    }
    s->allocs.push_back(slab);
    s->bytes += total;
    V.slab_bytes = (uint32_t)total;
    HIPCHK(hipMemset(slab, 0, total));
    int w = width, h = height;
    for (int l = 0; l < levels; l++) {
        uint8_t* d = slab + off[l];
        const size_t nb = (size_t)w * h * 3;
        if (l == 0 && jf) {  // decoded straight into level 0, or into the raw copy the undistortion reads
            const int rc = jpeg_frame_to_device(*jf, raw_copy ? raw_copy.p : d);
            if (rc != HPMVS_OK) return rc;
        }
        if (l == 0 && raw) {
            launch_undistort(raw, w, h, f, k1, d, nullptr);
            HIPCHK(hipGetLastError());
        } else if (l == 0) {
            if (!jf) HIPCHK(hipMemcpy(d, rgb_l0, nb, rgb_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        } else {
            launch_half_resize(V.pix[l - 1], V.w[l - 1], V.h[l - 1], d, nullptr);
            HIPCHK(hipGetLastError());
        }
        V.pix[l] = d; V.off[l] = (uint32_t)off[l]; V.w[l] = w; V.h[l] = h;
        w /= 2; h /= 2;
    }
    HIPCHK(hipDeviceSynchronize());
    memcpy(V.P0, cam->P0, sizeof(float) * 12);
    memcpy(V.center, cam->center, sizeof(float) * 4);
    for (int k = 0; k < 3; k++) { V.xaxis[k] = cam->xaxis[k]; V.yaxis[k] = cam->yaxis[k]; V.zaxis[k] = cam->zaxis[k]; }
    V.xaxis[3] = V.yaxis[3] = V.zaxis[3] = 0.0f;
    V.fsum = cam->fsum;
    V.n_levels = levels;
    s->view_set[view] = 1;
    return HPMVS_OK;
}

int hpmvs_scene_set_view(hpmvs_scene* s, int view, int width, int height, const uint8_t* rgb_l0, int rgb_on_device,
                         const hpmvs_camera* cam) {
    return set_view(s, view, width, height, rgb_l0, rgb_on_device, cam, 1.0f, 0.0f);
}

int hpmvs_scene_set_view_distorted(hpmvs_scene* s, int view, int width, int height, const uint8_t* rgb_raw,
                                   int rgb_on_device, const hpmvs_camera* cam, float f, float k1) {
    if (!undistort_args_ok(f, k1)) return fail(HPMVS_ERR_ARG, "scene_set_view_distorted: f must be finite and > 0, k1 finite");
    return set_view(s, view, width, height, rgb_raw, rgb_on_device, cam, f, k1);
}

int hpmvs_scene_get_level_jpeg(const hpmvs_scene* s, int view, int level, int quality, uint8_t* out, size_t cap, size_t* n) {
    if (!s || !n) return fail(HPMVS_ERR_ARG, "scene_get_level_jpeg: null argument");
    if (view < 0 || view >= s->n_views || !s->view_set[view]) return fail(HPMVS_ERR_ARG, "scene_get_level_jpeg: bad view");
    const DevView& V = s->hviews[view];
    if (level < 0 || level >= V.n_levels) return fail(HPMVS_ERR_ARG, "scene_get_level_jpeg: bad level");
    std::string err;
    const int rc = jpge::check_args(V.w[level], V.h[level], quality, &err);
    if (rc != jpge::kOk) return jpeg_enc_fail(rc, err);
    if (!out) {
        *n = jpge::encode_bound(V.w[level], V.h[level]);
        return HPMVS_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    return jpeg_encode_device(V.pix[level], V.w[level], V.h[level], quality, out, cap, n);
}

static int scene_set_view_jpeg_impl(hpmvs_scene* s, int view, const uint8_t* bytes, size_t n, const hpmvs_camera* cam, float f, float k1,
                                    int entropy, bool strict, int* used) {
    if (!s || !bytes || !cam) return fail(HPMVS_ERR_ARG, "scene_set_view_jpeg: null argument");
    if (!undistort_args_ok(f, k1)) return fail(HPMVS_ERR_ARG, "scene_set_view_jpeg: f must be finite and > 0, k1 finite");
    if (!jpeg_entropy_ok(entropy)) return fail(HPMVS_ERR_ARG, "scene_set_view_jpeg: bad entropy value");
    if (s->committed) return fail(HPMVS_ERR_STATE, "scene_set_view: scene already committed");
    if (view < 0 || view >= s->n_views) return fail(HPMVS_ERR_ARG, "scene_set_view_jpeg: bad view");
    JpegFile jf;
    if (const int rc = jpeg_open(bytes, n, jf)) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (const int rc = jpeg_decode_scan(jf, entropy, strict)) return rc;
    if (used) *used = jf.used;
    return set_view(s, view, jf.fr.W, jf.fr.H, nullptr, 0, cam, f, k1, &jf);
}

int hpmvs_scene_set_view_jpeg_ex(hpmvs_scene* s, int view, const uint8_t* bytes, size_t n, const hpmvs_camera* cam, float f, float k1,
                                 int entropy, int* used) {
    return scene_set_view_jpeg_impl(s, view, bytes, n, cam, f, k1, entropy, entropy == HPMVS_JPEG_ENTROPY_DEVICE, used);
}

int hpmvs_scene_set_view_jpeg(hpmvs_scene* s, int view, const uint8_t* bytes, size_t n, const hpmvs_camera* cam, float f, float k1) {
    return scene_set_view_jpeg_impl(s, view, bytes, n, cam, f, k1, jpeg_entropy_env(), false, nullptr);
}

int hpmvs_scene_set_covis(hpmvs_scene* s, int view, const int32_t* ids, int n) {
    if (!s || (n > 0 && !ids)) return fail(HPMVS_ERR_ARG, "scene_set_covis: null argument");
    if (s->committed) return fail(HPMVS_ERR_STATE, "scene_set_covis: scene already committed");
    if (view < 0 || view >= s->n_views || n < 0) return fail(HPMVS_ERR_ARG, "scene_set_covis: bad view");
    for (int k = 0; k < n; k++)
        if (ids[k] < 0 || ids[k] >= s->n_views) return fail(HPMVS_ERR_ARG, "scene_set_covis: id out of range");
    s->covis[view].assign(ids, ids + n);
    return HPMVS_OK;
}

int hpmvs_scene_commit(hpmvs_scene* s) {
    if (!s) return fail(HPMVS_ERR_ARG, "scene_commit: null scene");
    if (s->committed) return fail(HPMVS_ERR_STATE, "scene_commit: already committed");
    for (int v = 0; v < s->n_views; v++)
        if (!s->view_set[v]) return fail(HPMVS_ERR_STATE, "scene_commit: view " + std::to_string(v) + " not set");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMalloc((void**)&s->dviews, sizeof(DevView) * (size_t)s->n_views));
    HIPCHK(hipMemcpy(s->dviews, s->hviews.data(), sizeof(DevView) * (size_t)s->n_views, hipMemcpyHostToDevice));
    std::vector<int32_t> off(s->n_views + 1, 0), flat;
    for (int v = 0; v < s->n_views; v++) {
        off[v + 1] = off[v] + (int32_t)s->covis[v].size();
        flat.insert(flat.end(), s->covis[v].begin(), s->covis[v].end());
    }
    if (flat.empty()) flat.push_back(0);
    HIPCHK(hipMalloc((void**)&s->dcovis_off, sizeof(int32_t) * off.size()));
    HIPCHK(hipMemcpy(s->dcovis_off, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&s->dcovis, sizeof(int32_t) * flat.size()));
    HIPCHK(hipMemcpy(s->dcovis, flat.data(), sizeof(int32_t) * flat.size(), hipMemcpyHostToDevice));
    for (int k = 0; k < kQueueSlots; k++) HIPCHK(hipEventCreateWithFlags(&s->slot_done[k], hipEventDisableTiming));
    s->ws_bytes = (optimize_workspace_bytes(s->n_cus) + 255) & ~(size_t)255;
    HIPCHK(hipMalloc((void**)&s->dqueue[0], s->ws_bytes));  // the others on first concurrent use (acquire_workspace)
    HIPCHK(hipMemset(s->dqueue[0], 0, s->ws_bytes));
    HIPCHK(hipStreamSynchronize(nullptr));   // (the fills of the upload have run before any launch on another stream can start)
    s->n_queues = 1;
    s->bytes += s->ws_bytes;
    s->bytes += sizeof(DevView) * (size_t)s->n_views + sizeof(int32_t) * (off.size() + flat.size());
    s->committed = true;
    return HPMVS_OK;
}

int hpmvs_scene_destroy(hpmvs_scene* s) {
    if (!s) return HPMVS_OK;
    hipSetDevice(s->device);
    service_free(s);  // closes and drains the open batches of single-patch calls
    for (void* p : s->allocs) hipFree(p);
    if (s->depth_pool) hipFree(s->depth_pool);
    if (s->ddepth) hipFree(s->ddepth);
    if (s->dviews) hipFree(s->dviews);
    if (s->dcovis_off) hipFree(s->dcovis_off);
    if (s->dcovis) hipFree(s->dcovis);
    for (int k = 0; k < s->n_queues; k++) if (s->dqueue[k]) hipFree(s->dqueue[k]);
    for (auto& e : s->stage) {
        if (e.st) hipStreamDestroy(e.st);
        if (e.dev) hipFree(e.dev);
        if (e.host) hipHostFree(e.host);
    }
    for (int k = 0; k < kQueueSlots; k++) if (s->slot_done[k]) hipEventDestroy(s->slot_done[k]);
    if (s->ev0) hipEventDestroy(s->ev0);
    if (s->ev1) hipEventDestroy(s->ev1);
    delete s;
    return HPMVS_OK;
}

int hpmvs_scene_get_level(const hpmvs_scene* s, int view, int level, uint8_t* host_out, size_t cap, int* w, int* h) {
    if (!s || !w || !h) return fail(HPMVS_ERR_ARG, "scene_get_level: null argument");
    if (view < 0 || view >= s->n_views || !s->view_set[view]) return fail(HPMVS_ERR_ARG, "scene_get_level: bad view");
    const DevView& V = s->hviews[view];
    if (level < 0 || level >= V.n_levels) return fail(HPMVS_ERR_ARG, "scene_get_level: bad level");
    *w = V.w[level]; *h = V.h[level];
    const size_t nb = (size_t)V.w[level] * V.h[level] * 3;
    if (host_out) {
        if (cap < nb) return fail(HPMVS_ERR_ARG, "scene_get_level: buffer too small");
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipMemcpy(host_out, V.pix[level], nb, hipMemcpyDeviceToHost));
    }
    return HPMVS_OK;
}

size_t hpmvs_scene_bytes(const hpmvs_scene* s) { return s ? s->bytes : 0; }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// batch staging: host arrays <-> device arrays

namespace {

// hipMalloc / hipFree (and friends) wait for the device to be idle -- which it never is while single-patch callers keep an
// open batch running (a second one starts while the first drains).  Whatever allocates or frees while a scene is in use
// does it in an Exclusive scope: the scene lock (nobody can start an open batch meanwhile, service_open needs it) with
// the open batches ended and drained.  A host-staged call is in such a scope twice, briefly: for its allocations and for
// its frees (Call below); its copies, its launch and its wait run outside, so that concurrent big host batches against
// one scene overlap.
struct Exclusive {
    const hpmvs_scene* s;
    explicit Exclusive(const hpmvs_scene* s_) : s(s_) { if (s) { s->mu.lock(); (void)service_quiesce(s); } }
    ~Exclusive() { if (s) s->mu.unlock(); }
    Exclusive(const Exclusive&) = delete;
    Exclusive& operator=(const Exclusive&) = delete;
};

// Device address of [host, host + bytes) when the whole range lies in pinned host memory that is mapped into the GPU's
// address space (hipHostMalloc / hipHostRegister; torch's pin_memory()), else nullptr.  Such an array of a host-pointer
// call is used IN PLACE: the kernels read a patch's inputs once and write its outputs once, so they stream over PCIe while
// the kernel runs instead of costing a hipMalloc, two copies and a hipFree around it (C2: 222.3 -> 213.1 ms host to host
// against 212.1 ms of kernel).  HPMVS_ZERO_COPY=0 switches the detection off.
static void* mapped_host(const void* host, size_t bytes) {
    static const bool enabled = [] { const char* e = getenv("HPMVS_ZERO_COPY"); return !(e && e[0] == '0'); }();
    if (!enabled || !host || bytes == 0) return nullptr;
    void *d0 = nullptr, *d1 = nullptr;
    if (hipHostGetDevicePointer(&d0, const_cast<void*>(host), 0) != hipSuccess ||
        hipHostGetDevicePointer(&d1, const_cast<char*>((const char*)host + bytes - 1), 0) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error here
        return nullptr;
    }
    if ((const char*)d1 - (const char*)d0 != (ptrdiff_t)(bytes - 1)) return nullptr;
    // ... and both ends must belong to ONE allocation: two adjacent registrations could map their first and last byte the
    // right distance apart by accident.  Where the runtime cannot name the allocation the end-point test stands.
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d0) == hipSuccess && base && size) {
        if ((const char*)d0 < (const char*)base || (const char*)d0 + bytes > (const char*)base + size) return nullptr;
    } else {
        (void)hipGetLastError();
    }
    return d0;
}

DevBatch as_dev_batch(const hpmvs_patch_batch* b) {
    DevBatch d;
    memset(&d, 0, sizeof(d));
    d.n = b->n; d.max_images = b->max_images;
    d.center = b->center; d.normal = b->normal; d.scale = b->scale; d.n_images = b->n_images; d.images = b->images;
    d.ok = b->ok; d.color = b->color; d.ncc = b->ncc; d.fmin = b->fmin; d.x = b->x; d.result = b->result;
    d.nevals = b->nevals; d.stage = b->stage; d.ngrabs = b->ngrabs;
    return d;
}

// One call of a batch entry point, for both forms of its arguments.  With device pointers (on_device) every array is handed
// through as it is and nothing is allocated; with host pointers an array in pinned, mapped memory is used in place
// (mapped_host) and any other one travels through a device buffer of this call.  An entry point declares its arrays (batch /
// in / out / arr / scratch), calls begin(), launches once and returns finish(); of the form it is in it knows only what belongs
// to one form alone (filter_batch's offset verdict, init_patches_batch reading meas_off on the host, hpmvs_last_staging).
// A host-pointer call is in an Exclusive scope from its construction to begin() -- its allocations, and what drains the open
// batches ahead of it even when every array turns out to be pinned; a device-pointer call enters one only when it asks for
// scratch.  The destructor frees in a scope of its own.  The fills, the launch, the wait and the copies back run outside
// (two threads staging big host batches against one scene overlap them, 16 workspaces; they only take turns at hipMalloc /
// hipFree).  A failed allocation is remembered, the declarations after it do nothing and begin() returns it; every exit path
// frees what was allocated.
class Call {
public:
    // kCopyIn: an input, its contents travel to the device.  kZero: an output the kernel may leave untouched for some
    // patches (e.g. `color` of a failed one), which the call returns as 0; it decides for an array used in place -- a device
    // buffer that is not an input is always cleared.  kCopyBack: an output.
    enum : unsigned { kCopyIn = 1, kZero = 2, kCopyBack = 4 };
    // How a patch batch takes part.  kRead: its five input arrays.  kRefine (hpmvs_optimize_batch): the inputs travel both
    // ways, scale only in; the refinement kernel writes ok / fmin / x / result / nevals / stage / ngrabs of EVERY patch
    // (fetch and finish stages), so of the outputs only color and ncc are cleared.  kCreate: the call writes all fourteen
    // arrays, nothing travels in.
    enum Role { kRead, kRefine, kCreate };
    size_t staged_bytes = 0, mapped_bytes = 0;  // host arrays copied through device buffers / used in place

    Call(const hpmvs_scene* s, int on_device, hipStream_t st) : scene_(s), st_(st), device_(on_device != 0) {
        if (!device_) { scope_.emplace(s); arrs_.reserve(24); }
    }
    ~Call() {
        scope_.reset();
        if (!owned_) return;
        Exclusive ex(scene_);
        for (const Arr& a : arrs_)
            if (a.owned) hipFree(a.dev);
    }
    Call(const Call&) = delete;
    Call& operator=(const Call&) = delete;

    // the device address of an array of the caller's; a null or empty one stays null
    template <typename T>
    T* arr(const T* host, size_t count, unsigned flags) {
        if (device_) return const_cast<T*>(host);
        if (rc_ || !host || count == 0) return nullptr;
        const size_t bytes = sizeof(T) * count;
        if (void* m = mapped_host(host, bytes)) {
            mapped_bytes += bytes;
            if (flags & kZero) arrs_.push_back({m, nullptr, nullptr, bytes, false, true});
            return (T*)m;
        }
        staged_bytes += bytes;
        const bool input = (flags & kCopyIn) != 0;
        return (T*)alloc(bytes, input ? host : nullptr, !input, (flags & kCopyBack) ? const_cast<T*>(host) : nullptr);
    }
    template <typename T> T* in(const T* host, size_t count) { return arr(host, count, kCopyIn); }
    template <typename T> T* out(T* host, size_t count) { return arr(host, count, kZero | kCopyBack); }

    DevBatch batch(const hpmvs_patch_batch* b, Role role) {
        if (device_) return as_dev_batch(b);  // all fourteen pointers, whatever the role
        DevBatch d;
        memset(&d, 0, sizeof(d));
        d.n = b->n; d.max_images = b->max_images;
        const size_t n = (size_t)b->n;
        const unsigned io = role == kRead ? kCopyIn : role == kRefine ? kCopyIn | kCopyBack : kZero | kCopyBack;
        d.center = arr(b->center, 4 * n, io);
        d.normal = arr(b->normal, 4 * n, io);
        d.scale = arr(b->scale, n, role == kRefine ? kCopyIn : io);
        d.n_images = arr(b->n_images, n, io);
        d.images = arr(b->images, n * b->max_images, io);
        if (role == kRead) return d;
        const unsigned every = role == kRefine ? kCopyBack : kZero | kCopyBack;  // (written for every patch: no fill)
        d.ok = arr(b->ok, n, every);
        d.color = out(b->color, 3 * n);
        d.ncc = out(b->ncc, n);
        d.fmin = arr(b->fmin, n, every);
        d.x = arr(b->x, 3 * n, every);
        d.result = arr(b->result, n, every);
        d.nevals = arr(b->nevals, n, every);
        d.stage = arr(b->stage, n, every);
        d.ngrabs = arr(b->ngrabs, n, every);
        return d;
    }

    // device memory of the call's own, in both forms, never the caller's; freed with the call.  Also after begin(), then in a
    // scope of its own and without the zero fill.
    void* scratch(size_t bytes, bool zero = false) {
        if (rc_ || bytes == 0) return nullptr;
        const bool enter = !scope_;
        if (enter) scope_.emplace(scene_);
        void* p = alloc(bytes, nullptr, zero, nullptr);
        if (enter && begun_) scope_.reset();
        return p;
    }
    int error() const { return rc_; }

    // Leaves the Exclusive scope and issues the copies / zero fills of what was declared.  With a stream they go ON it (ordered
    // with the launch, and not waiting behind an open-batch kernel the way null-stream work can: ADVICE r4; a pageable source
    // is consumed before hipMemcpyAsync returns): hpmvs_optimize_batch and hpmvs_filter_batch.  The other entries fill on the
    // null stream and wait for it, as they always have; the launch stream is probably right for them too, but that changes
    // their order against open-batch kernels and is left for a change of its own.
    int begin(hipStream_t on = nullptr) {
        scope_.reset();
        begun_ = true;
        if (rc_) return rc_;
        bool null_fill = false;
        for (const Arr& a : arrs_) {
            if (!a.src && !a.zero) continue;
            if (on) {
                if (a.src) HIPCHK(hipMemcpyAsync(a.dev, a.src, a.bytes, hipMemcpyHostToDevice, on));
                else HIPCHK(hipMemsetAsync(a.dev, 0, a.bytes, on));
            } else if (a.src) { HIPCHK(hipMemcpy(a.dev, a.src, a.bytes, hipMemcpyHostToDevice)); null_fill = true; }
            else { HIPCHK(hipMemset(a.dev, 0, a.bytes)); null_fill = true; }
        }
        // a null-stream fill may return before it has run (hipMemset always, a copy from pageable memory once it is staged); the launch
        // that follows may go to a non-blocking stream of the caller's
        if (null_fill) HIPCHK(hipStreamSynchronize(nullptr));
        return HPMVS_OK;
    }

    // After the launch.  Host pointers: waits for the stream and copies back the outputs that went through device buffers
    // (those used in place are where they belong already).  Device pointers: returns at once, unless the call owns scratch
    // its kernels may still be using.
    int finish() {
        if (!device_ || owned_) HIPCHK(hipStreamSynchronize(st_));
        for (const Arr& a : arrs_)
            if (a.back) HIPCHK(hipMemcpy(a.back, a.dev, a.bytes, hipMemcpyDeviceToHost));
        return HPMVS_OK;
    }

private:
    struct Arr { void* dev; const void* src; void* back; size_t bytes; bool owned, zero; };  // src: copied in; back: copied back
    static int device_alloc(void** p, size_t bytes) {
        HIPCHK(hipMalloc(p, bytes));
        return HPMVS_OK;
    }
    void* alloc(size_t bytes, const void* src, bool zero, void* back) {
        void* p = nullptr;
        if ((rc_ = device_alloc(&p, bytes))) return nullptr;
        arrs_.push_back({p, src, back, bytes, true, zero});
        owned_ = true;
        return p;
    }
    const hpmvs_scene* scene_;  // null: a call against no scene (selftest), no lock to take
    hipStream_t st_;
    const bool device_;
    bool begun_ = false, owned_ = false;
    int rc_ = HPMVS_OK;
    std::optional<Exclusive> scope_;
    std::vector<Arr> arrs_;
};

int check_batch_shape(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* b) {
    if (!s || !o || !b) return fail(HPMVS_ERR_ARG, "null scene/options/batch");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "scene not committed");
    if (b->n < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "bad n/max_images");
    if (o->MAXLEVEL < 1 || o->MAXLEVEL >= HPMVS_MAX_LEVELS) return fail(HPMVS_ERR_ARG, "MAXLEVEL out of range");
    // a negative level would index the per-level tables with a negative subscript (addImages); an image-count floor
    // below 1 would let an empty list reach setINCCs (the reference's addImages fails on an empty list regardless)
    if (o->MINLEVEL < 0 || o->MINLEVEL > o->MAXLEVEL) return fail(HPMVS_ERR_ARG, "MINLEVEL out of range");
    if (o->MIN_IMAGES_PER_PATCH < 1) return fail(HPMVS_ERR_ARG, "MIN_IMAGES_PER_PATCH must be >= 1");
    // sampleTexture reads pyramid levels up to MAXLEVEL - 1 (PatchOptimizer.cpp:487); the device forms the level's address
    // arithmetically inside the view's slab (prep_from_view), so a view with fewer levels must be refused here
    for (int v = 0; v < s->n_views; v++)
        if (s->hviews[v].n_levels < o->MAXLEVEL) return fail(HPMVS_ERR_ARG, "options.MAXLEVEL exceeds the pyramid levels of a view");
    return HPMVS_OK;
}

int check_batch(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* b) {
    const int rc = check_batch_shape(s, o, b);
    if (rc) return rc;
    if (b->n > 0 && (!b->center || !b->normal || !b->scale || !b->n_images || !b->images))
        return fail(HPMVS_ERR_ARG, "batch input arrays missing");
    return HPMVS_OK;
}

DevScene dev_scene(const hpmvs_scene* s) {
    DevScene sc;
    sc.views = s->dviews; sc.covis_off = s->dcovis_off; sc.covis = s->dcovis; sc.n_views = s->n_views;
    // level thresholds (dev_types.h): smallest double r with (float)log2(r) >= k + 0.5, by bisection on the bit pattern
    static const std::vector<double> thr = [] {
        std::vector<double> t(kMaxLevels);
        for (int k = 0; k < kMaxLevels; k++) {
            const float target = (float)k + 0.5f;
            double lo = std::ldexp(1.0, k), hi = std::ldexp(1.0, k + 1);  // (float)log2(lo) = k < target <= k + 1 = (float)log2(hi)
            unsigned long long a, b;
            memcpy(&a, &lo, 8); memcpy(&b, &hi, 8);
            while (b - a > 1) {
                const unsigned long long m = a + (b - a) / 2;
                double r; memcpy(&r, &m, 8);
                if ((float)std::log2(r) >= target) b = m; else a = m;
            }
            memcpy(&t[k], &b, 8);
        }
        return t;
    }();
    for (int k = 0; k < kMaxLevels; k++) sc.lvl_thr[k] = thr[k];
    return sc;
}

}  // namespace

// One refinement launch on `st` (call with s->mu held): picks the kernel, hands out / zeroes its workspace and
// brackets it with the scene's event pair.
static int enqueue_refinement(const hpmvs_scene* s, const DevOptions& d, const DevBatch& batch, hipStream_t st) {
    int rc;
    // A batch launch needs whole CUs (one workgroup takes a CU's LDS), an open batch holds a quarter of every CU for as
    // long as single-patch callers keep it open -- and its long-running kernel may sit in the very hardware queue this
    // launch's packets go to.  So the open batches end first: closed (their published patches are still finished, a few
    // milliseconds) and drained.  Callers that come later start a new one, which queues behind this launch (service_open).
    if ((rc = service_quiesce(s))) return rc;
    {
        Workspace ws(s, st);
        if (ws.rc) return ws.rc;
        int32_t* q = ws.q;
        HIPCHK(hipMemsetAsync(q, 0, kQueueSlotBytes, st));
        HIPCHK(hipEventRecord(s->ev0, st));
        launch_optimize(dev_scene(s), d, batch, q, s->n_cus, st);
        s->last_ws = q;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->ev1, st));
    }
    s->timed = true;
    return HPMVS_OK;
}
// ---- multi-GPU exchange ------------------------------------------------------------------------------------------
static_assert(sizeof(hpmvs_record) == 192, "hpmvs_record is 192 bytes");
extern "C" int hpmvs_pack_records(const hpmvs_patch_batch* b, hpmvs_record* records, void* stream) {
    if (!b || b->n < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "pack_records: bad batch");
    if (b->n > 0 && (!records || !b->center || !b->normal || !b->scale || !b->n_images || !b->images))
        return fail(HPMVS_ERR_ARG, "pack_records: missing array");
    launch_pack_records(as_dev_batch(b), records, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HPMVS_OK;
}
extern "C" int hpmvs_unpack_records(const hpmvs_record* records, int n, hpmvs_patch_batch* b, void* stream) {
    if (!b || n < 0 || b->n < n || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "unpack_records: bad batch");
    if (n > 0 && (!records || !b->center || !b->normal || !b->scale || !b->n_images || !b->images))
        return fail(HPMVS_ERR_ARG, "unpack_records: missing array");
    launch_unpack_records(records, n, as_dev_batch(b), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HPMVS_OK;
}
static_assert(sizeof(hpmvs_record_tail) == 392, "hpmvs_record_tail is 392 bytes");
extern "C" int hpmvs_pack_record_tails(const hpmvs_patch_batch* b, hpmvs_record_tail* tails, int32_t cap, int32_t* n_tails, void* stream) {
    if (!b || !n_tails || b->n < 0 || cap < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "pack_record_tails: bad batch");
    *n_tails = 0;
    if (b->n == 0 || b->max_images <= HPMVS_RECORD_IMAGES) return HPMVS_OK;   // (rows of up to 64 ids have no tails)
    if (!b->n_images || !b->images || (cap > 0 && !tails)) return fail(HPMVS_ERR_ARG, "pack_record_tails: missing array");
    hipStream_t st = (hipStream_t)stream;
    const size_t nblocks = ((size_t)b->n + 63) / 64;
    int32_t* scratch = nullptr;
    HIPCHK(hipMalloc((void**)&scratch, sizeof(int32_t) * (nblocks + 1)));
    launch_pack_record_tails(as_dev_batch(b), tails, cap, scratch, scratch + nblocks, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(n_tails, scratch + nblocks, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(scratch);
    if (e != hipSuccess) return fail(HPMVS_ERR_HIP, std::string("pack_record_tails: ") + hipGetErrorString(e));
    if (*n_tails > cap) return fail(HPMVS_ERR_ARG, "pack_record_tails: " + std::to_string(*n_tails) + " tails do not fit the " + std::to_string(cap) + " handed over");
    return HPMVS_OK;
}
extern "C" int hpmvs_unpack_record_tails(const hpmvs_record_tail* tails, int32_t n_tails, int32_t patch_offset, hpmvs_patch_batch* b, void* stream) {
    if (!b || n_tails < 0 || b->n < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "unpack_record_tails: bad batch");
    if (n_tails == 0) return HPMVS_OK;
    if (!tails || !b->images) return fail(HPMVS_ERR_ARG, "unpack_record_tails: missing array");
    launch_unpack_record_tails(tails, n_tails, patch_offset, as_dev_batch(b), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HPMVS_OK;
}
// ncclAllGather(sendbuff, recvbuff, sendcount, datatype, comm, stream); ncclUint8 = 1, ncclSuccess = 0 (rccl.h)
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static nccl_allgather_fn find_allgather() {
    static nccl_allgather_fn fn = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        // HPMVS_RCCL_LIBRARY names the library to take ncclAllGather from (an application that links its own build of
        // RCCL under another name); otherwise the RCCL already in the process (the communicator's own), then the
        // system's librccl
        void* sym = nullptr;
        if (const char* named = getenv("HPMVS_RCCL_LIBRARY")) {
            if (void* h = dlopen(named, RTLD_NOW | RTLD_GLOBAL)) sym = dlsym(h, "ncclAllGather");
        } else {
            sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
            if (!sym) {
                void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
                if (h) sym = dlsym(h, "ncclAllGather");
            }
        }
        fn = (nccl_allgather_fn)sym;
    });
    return fn;
}
extern "C" int hpmvs_allgather_records(void* nccl_comm, const hpmvs_record* send, size_t count, hpmvs_record* recv, void* stream) {
    if (!nccl_comm || (count > 0 && (!send || !recv))) return fail(HPMVS_ERR_ARG, "allgather_records: null argument");
    nccl_allgather_fn fn = find_allgather();
    if (!fn) return fail(HPMVS_ERR_STATE, "allgather_records: RCCL (ncclAllGather) not found in the process, as librccl.so.1 nor as $HPMVS_RCCL_LIBRARY");
    if (count > 0) {
        // both buffers must be device memory of ONE device (the communicator's): a host pointer or a buffer of another
        // GPU would fault inside the collective, on every rank
        hipPointerAttribute_t as{}, ar{};
        if (hipPointerGetAttributes(&as, send) != hipSuccess || hipPointerGetAttributes(&ar, recv) != hipSuccess ||
            as.type != hipMemoryTypeDevice || ar.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(HPMVS_ERR_ARG, "allgather_records: send / recv must be device memory");
        }
        if (as.device != ar.device)
            return fail(HPMVS_ERR_ARG, "allgather_records: send is on device " + std::to_string(as.device) + ", recv on device " + std::to_string(ar.device));
    }
    const int r = fn(send, recv, count * sizeof(hpmvs_record), /*ncclUint8*/ 1, nccl_comm, (hipStream_t)stream);
    if (r != 0) return fail(HPMVS_ERR_HIP, "ncclAllGather failed with ncclResult_t " + std::to_string(r));
    return HPMVS_OK;
}

extern "C" int hpmvs_selftest_bobyqa(int device, int n, const int32_t* kind, const double* params, const double* x0,
                                     const double* lb, const double* ub, int maxeval, double* xfinal, double* minf,
                                     int32_t* result, int32_t* nevals, int32_t* rescue_calls, double* trace, int trace_cap) {
    if (n < 0 || (n > 0 && (!kind || !params || !x0 || !lb || !ub || !xfinal || !minf || !result || !nevals || !rescue_calls)))
        return fail(HPMVS_ERR_ARG, "selftest_bobyqa: missing array");
    if (trace && trace_cap < 1) return fail(HPMVS_ERR_ARG, "selftest_bobyqa: trace_cap");
    if (const int rc = use_device(device, "selftest_bobyqa")) return rc;
    if (n == 0) return HPMVS_OK;
    Call c(nullptr, 0, nullptr);
    const size_t N = (size_t)n;
    const int32_t* dkind = c.in(kind, N);
    const double *dpar = c.in(params, 8 * N), *dx0 = c.in(x0, 3 * N), *dlb = c.in(lb, 3 * N), *dub = c.in(ub, 3 * N);
    double *dxf = c.out(xfinal, 3 * N), *dmin = c.out(minf, N);
    int32_t *drc = c.out(result, N), *dne = c.out(nevals, N), *dres = c.out(rescue_calls, N);
    double* dtr = c.out(trace, 4 * N * (size_t)trace_cap);
    double* dcold = (double*)c.scratch(sizeof(double) * selftest_cold_doubles(n), /*zero=*/true);
    int rc;
    if ((rc = c.begin())) return rc;
    launch_selftest(n, dkind, dpar, dx0, dlb, dub, maxeval, dxf, dmin, drc, dne, dres, dtr, trace_cap, dcold, nullptr);
    HIPCHK(hipGetLastError());
    return c.finish();
}

// ---- the patch cloud as DynOctTree::toExtPly's file (kernel_ply.hip, ply_text.hpp) ---------------------------------------------
// One implementation under hpmvs_ply_ext_batch and hpmvs_ply_ext_timed (ms != nullptr: host pointers, the null stream, six stage
// times).  The header is built on the host; the body's lengths, places and bytes on the device; one read of 16 bytes brings back
// the body's length and the error word.
static int ply_ext(const char* who, int device, const hpmvs_patch_batch* b, const int32_t* order, int n_rows, int flags, uint8_t* out, size_t cap,
                   size_t* n, int on_device, hipStream_t st, float* ms) {
    const std::string w(who);
    if (!b || !n) return fail(HPMVS_ERR_ARG, w + ": null argument");
    if (flags & ~ply::kAllFlags) return fail(HPMVS_ERR_ARG, w + ": unknown flag bits");
    if (!out && cap) return fail(HPMVS_ERR_ARG, w + ": a capacity without an output buffer");
    if (b->n < 0 || b->max_images < 0) return fail(HPMVS_ERR_ARG, w + ": bad n/max_images");
    if (order && n_rows < 0) return fail(HPMVS_ERR_ARG, w + ": negative n_rows");
    const int R = order ? n_rows : b->n;
    const bool vis = (flags & ply::kVisibility) != 0;
    if (R > 0 && (!b->center || !b->color || ((flags & ply::kNormal) && !b->normal) || ((flags & ply::kScale) && !b->scale) ||
                  (vis && (!b->n_images || (b->max_images > 0 && !b->images)))))
        return fail(HPMVS_ERR_ARG, w + ": batch arrays missing");
    if (const int rc = use_device(device, who)) return rc;
    const std::string head = ply::header(R, flags);
    if (ms) for (int k = 0; k < 6; k++) ms[k] = 0.0f;
    if (R == 0) {
        *n = head.size();
        if (!out) return HPMVS_OK;
        if (cap < *n) return fail(HPMVS_ERR_ARG, w + ": output buffer too small (" + std::to_string(*n) + " bytes needed)");
        memcpy(out, head.data(), head.size());
        return HPMVS_OK;
    }
    EventMarks ev(7, ms != nullptr);
    HIPCHK(ev.created());
    HIPCHK(ev.mark(0));
    Call c(nullptr, on_device, st);
    const size_t N = (size_t)b->n, rows = (size_t)R, n_len = 2 * rows + 1;
    PlyRows A;
    memset(&A, 0, sizeof(A));
    A.n = b->n; A.max_images = b->max_images; A.n_rows = R; A.flags = flags;
    A.center = c.in(b->center, 4 * N);
    A.color = c.in(b->color, 3 * N);
    if (flags & ply::kNormal) A.normal = c.in(b->normal, 4 * N);
    if (flags & ply::kScale) A.scale = c.in(b->scale, N);
    if (vis) { A.n_images = c.in(b->n_images, N); A.images = c.in(b->images, N * (size_t)b->max_images); }
    A.order = order ? c.in(order, rows) : nullptr;
    size_t scan_bytes = 0;
    HIPCHK((hipError_t)jpeg_enc_scan(nullptr, &scan_bytes, nullptr, nullptr, n_len, nullptr));
    Layout L;
    // (the scan's last entry and the error word lie side by side: one read brings both back)
    const size_t o_len = L.take(n_len * 8), o_offs = L.take((n_len + 1) * 8), o_temp = L.take(scan_bytes),
                 o_rec = L.take((flags & ply::kBinary) ? 0 : ply::kRowRecords * rows * sizeof(uint32_t));
    uint8_t* work = (uint8_t*)c.scratch(L.total);
    int rc;
    if ((rc = c.begin(st))) return rc;
    HIPCHK(ev.mark(1));
    unsigned long long *d_len = (unsigned long long*)(work + o_len), *d_offs = (unsigned long long*)(work + o_offs);
    A.len = d_len;
    A.rec = (uint32_t*)(work + o_rec);
    A.err = (unsigned int*)(d_offs + n_len);
    HIPCHK(hipMemsetAsync(d_len + (n_len - 1), 0, 8, st));
    HIPCHK(hipMemsetAsync(d_offs + n_len, 0xFF, 8, st));
    launch_ply_len(A, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(2));
    HIPCHK((hipError_t)jpeg_enc_scan(work + o_temp, &scan_bytes, d_len, d_offs, n_len, st));
    unsigned long long back[2] = {0ull, 0ull};   // the body's length; the error word in the low half of the second
    HIPCHK(hipMemcpyAsync(back, d_offs + (n_len - 1), 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.mark(3));
    const unsigned int err = (unsigned int)(back[1] & 0xFFFFFFFFull);
    if (err != 0xFFFFFFFFu) {
        const std::string row = w + ": row " + std::to_string(err >> 1);
        return fail(HPMVS_ERR_ARG, (err & 1u) ? row + " holds an n_images outside [0, " + std::to_string(b->max_images) + "]"
                                              : row + " names a patch outside [0, " + std::to_string(b->n) + ")");
    }
    const size_t body = (size_t)back[0];
    *n = head.size() + body;
    if (!out) return c.finish();
    if (cap < *n) return fail(HPMVS_ERR_ARG, w + ": output buffer too small (" + std::to_string(*n) + " bytes needed)");
    uint8_t* d_body = (uint8_t*)c.scratch(body);
    if ((rc = c.error())) return rc;
    launch_ply_vertex(A, d_offs, d_body, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(4));
    launch_ply_list(A, d_offs, d_body, st);
    HIPCHK(hipGetLastError());
    HIPCHK(ev.mark(5));
    HIPCHK(hipMemcpyAsync(out + head.size(), d_body, body, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ev.mark(6));
    memcpy(out, head.data(), head.size());
    if (ms) {
        HIPCHK(ev.sync(6));
        for (int k = 0; k < 6; k++) HIPCHK(ev.elapsed(k, k + 1, &ms[k]));
    }
    return c.finish();
}

extern "C" int hpmvs_ply_ext_batch(int device, const hpmvs_patch_batch* b, const int32_t* order, int n_rows, int flags, uint8_t* out, size_t cap,
                                   size_t* n, int on_device, void* stream) {
    return ply_ext("ply_ext_batch", device, b, order, n_rows, flags, out, cap, n, on_device, (hipStream_t)stream, nullptr);
}
extern "C" int hpmvs_ply_ext_timed(int device, const hpmvs_patch_batch* b, const int32_t* order, int n_rows, int flags, uint8_t* out, size_t cap,
                                   size_t* n, float* ms) {
    if (!ms) return fail(HPMVS_ERR_ARG, "ply_ext_timed: null argument");
    return ply_ext("ply_ext_timed", device, b, order, n_rows, flags, out, cap, n, 0, nullptr, ms);
}

// ---- pooled staging of a small host batch -------------------------------------------------------------------------
namespace {
struct PoolLayout {
    size_t off_center, off_normal, off_scale, off_nimg, off_images, in_bytes;
    size_t off_ok, off_color, off_ncc, off_fmin, off_x, off_result, off_nevals, off_stage, off_ngrabs, total;
};
PoolLayout pool_layout(size_t n, size_t m) {
    PoolLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
    L.off_center = take(16 * n); L.off_normal = take(16 * n); L.off_scale = take(4 * n); L.off_nimg = take(4 * n);
    L.off_images = take(4 * n * m);
    L.in_bytes = o;
    L.off_ok = take(n); L.off_color = take(12 * n); L.off_ncc = take(4 * n); L.off_fmin = take(8 * n); L.off_x = take(24 * n);
    L.off_result = take(4 * n); L.off_nevals = take(4 * n); L.off_stage = take(4 * n); L.off_ngrabs = take(4 * n);
    L.total = o;
    return L;
}
}  // namespace

// ------------------------------------------------------------------------------------------
// OPEN BATCH: the service behind single-patch host calls.
//
// The reference's callers hand over ONE patch per optimize() call from many host threads (Scene.cpp:166-167,
// CellProcessor.cpp:129,256).  A launch per call costs a kernel start and two PCIe copies; a launch per group of
// callers (the combiner of round 2) makes everybody wait for the slowest patch of the group (450 evaluations against a
// mean of 88).  Here ONE long-running launch serves them all: its patch arrays live in host-mapped memory and have
// room for kCap patches; a calling thread appends its patch, publishes the new count (ctrl[0]) and spins on its own
// done flag, which the kernel sets as soon as that patch's results are visible to the host -- so a caller waits for
// its own patch only.  The launch is closed (ctrl[1] = 1, the kernel drains and exits) when nobody is waiting any
// more, when its room is used up, or when the options change; a second Service object takes over meanwhile.
// Results are those of any other launch: patches are independent.
// HPMVS_SERVICE_STATS=1: where the time of a call goes (printed at exit)
static std::atomic<long long> g_svc_ns_hold{0}, g_svc_ns_acq{0}, g_svc_slow{0}, g_svc_acq_long{0}, g_svc_ns_acq_long{0};
static std::atomic<long long> g_svc_calls{0}, g_svc_ns_lock{0}, g_svc_ns_wait{0}, g_svc_ns_total{0}, g_svc_opens{0};
static bool service_stats() {
    static const bool on = [] {
        const char* e = getenv("HPMVS_SERVICE_STATS");
        const bool v = e && e[0] == '1';
        if (v) atexit([] {
            const double c = (double)std::max<long long>(1, g_svc_calls.load());
            fprintf(stderr, "hpmvs service: %lld calls, %lld launches; per call: submit (lock + copy) %.1f us of which the lock is held %.1f us [to get the submission lock %.1f us on average; %lld calls waited > 200 us for it, %.0f us each: behind a thread that was starting a launch; %lld launches started], wait for the device %.1f us, total %.1f us\n",
                    g_svc_calls.load(), g_svc_opens.load(), g_svc_ns_lock.load() / c / 1e3, g_svc_ns_hold.load() / c / 1e3, g_svc_ns_acq.load() / c / 1e3, g_svc_acq_long.load(), g_svc_ns_acq_long.load() / 1e3 / (double)std::max<long long>(1, g_svc_acq_long.load()), g_svc_slow.load(), g_svc_ns_wait.load() / c / 1e3, g_svc_ns_total.load() / c / 1e3);
        });
        return v;
    }();
    return on;
}

struct hpmvs_scene::Service {
    static constexpr int kCap = 16384;      // patches per open batch
    static constexpr int kLanes = 2;        // patches per wavefront (few: latency first)
    hipStream_t st = nullptr;
    char* host = nullptr;                   // host-mapped, coherent: IN records, OUT records, ctrl words, done flags
    int32_t* ws = nullptr;                  // launch workspace + the slots' staging records
    size_t ws_bytes = 0, stage_off = 0;
    int wgs = 0;
    uint32_t* in = nullptr;                 // kCap x kSvcInDwords
    uint32_t* out = nullptr;                // kCap x kSvcOutDwords
    volatile int32_t* ctrl = nullptr;
    volatile int32_t* done = nullptr;
    int published = 0;
    unsigned gen = 0;                       // launch generation (service_open increments it): a closer ends only the launch it published into
    std::atomic<int> outstanding{0};        // published patches whose owner has not picked up the results yet
    bool open = false, running = false;
    hpmvs_options opts;
};

static void service_close(hpmvs_scene::Service& S) {  // call with svc_mu held
    if (S.open) {
        std::atomic_thread_fence(std::memory_order_release);
        S.ctrl[1] = 1;
        S.open = false;
    }
}
static int service_wait_drained(hpmvs_scene::Service& S) {
    if (S.running) {
        HIPCHK(hipStreamSynchronize(S.st));
        S.running = false;
    }
    return HPMVS_OK;
}
static void service_close_all(const hpmvs_scene* s) {
    std::lock_guard<std::mutex> lk(s->svc_mu);
    for (int k = 0; k < 2; k++)
        if (s->svc[k]) service_close(*s->svc[k]);
}
// closes and drains every open batch of the scene (before anything that synchronises the whole device)
static int service_quiesce(const hpmvs_scene* s) {
    std::lock_guard<std::mutex> lk(s->svc_mu);
    for (int k = 0; k < 2; k++)
        if (s->svc[k]) {
            service_close(*s->svc[k]);
            int rc = service_wait_drained(*s->svc[k]);
            if (rc) return rc;
        }
    return HPMVS_OK;
}
// stream, host-mapped record area and launch workspace of one open-batch object (~12 MB pinned + the workspace: ~12 ms)
static int service_alloc(const hpmvs_scene* s, hpmvs_scene::Service& S) {
    using Service = hpmvs_scene::Service;
    if (S.st) return HPMVS_OK;
    const size_t in_bytes = sizeof(uint32_t) * kSvcInDwords * (size_t)Service::kCap;
    const size_t out_bytes = sizeof(uint32_t) * kSvcOutDwords * (size_t)Service::kCap;
    {
        S.wgs = s->n_cus;  // one workgroup per CU: batch launches keep three quarters of every CU
        if (const char* e = getenv("HPMVS_SERVICE_WGS")) S.wgs = atoi(e) > 0 ? atoi(e) : S.wgs;  // (experiments)
        S.stage_off = (optimize_workspace_bytes_for(S.wgs) + 255) & ~(size_t)255;
        S.ws_bytes = S.stage_off + optimize_stage_bytes_for(S.wgs);
        hipStream_t st = nullptr; char* hv = nullptr; int32_t* wv = nullptr;
        const size_t hbytes = in_bytes + out_bytes + 256 + sizeof(int32_t) * (size_t)Service::kCap;
        bool good = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
        good = good && hipHostMalloc((void**)&hv, hbytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
        good = good && hipMalloc((void**)&wv, S.ws_bytes) == hipSuccess;
        if (!good) {
            if (wv) hipFree(wv);
            if (hv) hipHostFree(hv);
            if (st) hipStreamDestroy(st);
            return fail(HPMVS_ERR_HIP, "cannot allocate the open batch of single-patch calls");
        }
        S.st = st; S.host = hv; S.ws = wv;
        S.in = (uint32_t*)hv; S.out = (uint32_t*)(hv + in_bytes);
        S.ctrl = (volatile int32_t*)(hv + in_bytes + out_bytes);
        S.done = (volatile int32_t*)(hv + in_bytes + out_bytes + 256);
    }
    return HPMVS_OK;
}
static int service_open(const hpmvs_scene* s, hpmvs_scene::Service& S, const hpmvs_options* o) {  // s->mu and svc_mu held
    using Service = hpmvs_scene::Service;
    int rc = service_wait_drained(S);
    if (rc) return rc;
    // the owners of the previous generation's patches read their results from S.host: not before they are done
    while (S.outstanding.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    if ((rc = service_alloc(s, S))) return rc;
    memset((void*)S.ctrl, 0, 256 + sizeof(int32_t) * (size_t)Service::kCap);  // ctrl + done flags
    S.opts = *o;
    S.published = 0; S.outstanding.store(0);
    S.gen++;
    DevBatch D;
    memset(&D, 0, sizeof(D));
    D.n = Service::kCap; D.max_images = HPMVS_FAST_IMAGES;   // (the open batch's records hold 64 ids)
    // (unified addressing: the host pointer is the device pointer of mapped memory)
    D.svc_in = (const unsigned long long*)S.in; D.svc_out = S.out; D.svc_stage = (uint32_t*)((char*)S.ws + S.stage_off);
    D.svc_ctrl = (const int32_t*)S.ctrl; D.svc_done = (int32_t*)S.done; D.svc_lanes = Service::kLanes;
    if (const char* e = getenv("HPMVS_SERVICE_LANES")) D.svc_lanes = atoi(e) > 0 ? atoi(e) : D.svc_lanes;  // (experiments)
    HIPCHK(hipMemsetAsync(S.ws, 0, kQueueSlotBytes, S.st));
    // behind every batch launch enqueued so far (they need whole CUs and must not find this launch in their way; launches
    // enqueued later end it: enqueue_refinement)
    for (int k = 0; k < kQueueSlots; k++)
        if (s->slot_used[k]) HIPCHK(hipStreamWaitEvent(S.st, s->slot_done[k], 0));
    launch_optimize_service(dev_scene(s), make_dev_options(o), D, S.ws, S.wgs, S.st);
    HIPCHK(hipGetLastError());
    S.open = true; S.running = true;
    g_svc_opens++;
    return HPMVS_OK;
}

static void service_free(hpmvs_scene* s) {
    service_quiesce(s);
    for (int k = 0; k < 2; k++)
        if (s->svc[k]) {
            if (s->svc[k]->ws) hipFree(s->svc[k]->ws);
            if (s->svc[k]->host) hipHostFree(s->svc[k]->host);
            if (s->svc[k]->st) hipStreamDestroy(s->svc[k]->st);
            delete s->svc[k];
            s->svc[k] = nullptr;
        }
}

static bool service_enabled() {
    static const bool on = [] { const char* e = getenv("HPMVS_SERVICE"); return !(e && e[0] == '0'); }();
    return on;
}

// hpmvs_optimize_batch for a handful of host-resident patches (the unchanged callers' optimize() = batch of one)
static int optimize_through_service(const hpmvs_scene* s, const hpmvs_options* o, hpmvs_patch_batch* b) {
    using Service = hpmvs_scene::Service;
    const int n = b->n, m = b->max_images;
    const bool stats = service_stats();
    const auto t_in = std::chrono::steady_clock::now();
    Service* S = nullptr;
    int k0 = 0;
    unsigned my_gen = 0;
    auto usable = [&](const Service* cur) {
        return cur && cur->open && cur->published + n <= Service::kCap && memcmp(&cur->opts, o, sizeof(*o)) == 0;
    };
    for (;;) {
        {
            // the critical section is a few microseconds; a contended futex hand-over costs far more than that (256
            // callers: ~1 ms per submission in the convoy), so try for a moment before queueing up
            bool got = false;
            for (int spin = 0; spin < 400 && !(got = s->svc_mu.try_lock()); spin++) __builtin_ia32_pause();
            if (!got) s->svc_mu.lock();
        }
        if (usable(s->svc[0] ? s->svc[s->svc_cur] : nullptr)) break;  // (svc_mu stays locked)
        s->svc_mu.unlock();
        g_svc_slow++;
        // No open batch that takes this patch: start one -- under the scene lock first (lock order: mu, then svc_mu), so
        // that it is ordered against batch launches: one enqueued before waits on the stream, one enqueued after ends it.
        std::lock_guard<std::recursive_mutex> l1(s->mu);
        std::lock_guard<std::mutex> l2(s->svc_mu);
        if (!s->svc[0]) {
            // both objects get their memory NOW: the first caller that finds the current batch closed (full, other options, ended by
            // a batch launch) would otherwise stall every other caller for the ~12 ms the second object's allocations take
            // (measured: 257 of the first calls of a 256-thread loop waited 14.7 ms each, profiles/r05/callers_host_side.txt)
            s->svc[0] = new Service(); s->svc[1] = new Service();
            int rc0 = service_alloc(s, *s->svc[0]);
            if (!rc0) rc0 = service_alloc(s, *s->svc[1]);
            if (rc0) return rc0;
        }
        Service* cur = s->svc[s->svc_cur];
        if (usable(cur)) continue;  // somebody else did meanwhile
        service_close(*cur);
        s->svc_cur ^= 1;
        cur = s->svc[s->svc_cur];
        service_close(*cur);  // (can only be open if the options flipped twice)
        const int rc = service_open(s, *cur, o);
        if (rc) return rc;
    }
    {
        std::lock_guard<std::mutex> lk(s->svc_mu, std::adopt_lock);
        const auto t_held = std::chrono::steady_clock::now();
        if (stats) {
            const long long a = std::chrono::duration_cast<std::chrono::nanoseconds>(t_held - t_in).count();
            g_svc_ns_acq += a;
            if (a > 200000) { g_svc_acq_long++; g_svc_ns_acq_long += a; }  // (waited behind somebody who was opening a launch)
        }
        struct Hold { bool on; std::chrono::steady_clock::time_point t0; ~Hold() { if (on) g_svc_ns_hold += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); } } hold{stats, t_held};
        Service* cur = s->svc[s->svc_cur];
        S = cur;
        my_gen = S->gen;
        k0 = S->published;
        for (int i = 0; i < n; i++) {
            uint32_t* rec = S->in + (size_t)(k0 + i) * kSvcInDwords;
            memcpy(rec + 0, b->center + 4 * i, 12); memcpy(rec + 3, b->scale + i, 4);
            memcpy(rec + 4, b->normal + 4 * i, 12);
            // a list longer than the caller's row cannot come back: failed like every other launch does (stage 100)
            const int32_t ni = b->n_images[i] > m ? (int32_t)(HPMVS_FAST_IMAGES + 1) : b->n_images[i];
            memcpy(rec + 7, &ni, 4);
            memcpy(rec + 8, b->images + (size_t)i * m, 4 * (size_t)m);
        }
        std::atomic_thread_fence(std::memory_order_release);
        S->ctrl[0] = k0 + n;  // published
        S->published += n; S->outstanding.fetch_add(n);
    }
    const auto t_sub = std::chrono::steady_clock::now();
    static const long poll_us = [] { const char* e = getenv("HPMVS_SERVICE_POLL_US"); return e ? atol(e) : 50L; }();
    // wait for my own patches only
    int rc = HPMVS_OK;
    for (int i = 0; i < n && rc == HPMVS_OK; i++) {
        const int k = k0 + i;
        unsigned spins = 0;
        auto t_check = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
        // a patch is at most 1000 evaluation rounds of well under a millisecond; far beyond that the device is not
        // making progress and the caller gets an error instead of waiting for ever
        static const long limit_s = [] { const char* e = getenv("HPMVS_SERVICE_TIMEOUT_S"); return e && atol(e) > 0 ? atol(e) : 120L; }();
        const auto t_limit = std::chrono::steady_clock::now() + std::chrono::seconds(limit_s);
        while (S->done[k] == 0) {
            // Poll gently: the flags live in host memory that the GPU writes over PCIe, and hundreds of cores reading
            // those lines back to back delay exactly those writes and the device's reads of the progress words
            // (256 threads spinning: 6.7 k patches/s; sleeping 50 us between polls: 50 k).  A patch
            // needs milliseconds on the device, so the sleep costs nothing.
            ++spins;
            if (poll_us > 0) { struct timespec ts = {0, poll_us * 1000L}; nanosleep(&ts, nullptr); }
            else if (spins < 2000) { __builtin_ia32_pause(); continue; }
            else std::this_thread::yield();
            if ((spins & 0xfff) == 0 && std::chrono::steady_clock::now() > t_check) {
                // the launch must still be running while my flag is down
                const hipError_t q = hipStreamQuery(S->st);
                if (q != hipErrorNotReady && S->done[k] == 0) { rc = fail(HPMVS_ERR_HIP, "open batch ended without finishing a published patch"); break; }
                if (std::chrono::steady_clock::now() > t_limit) { rc = fail(HPMVS_ERR_HIP, "open batch: a published patch was not finished within " + std::to_string(limit_s) + " s (HPMVS_SERVICE_TIMEOUT_S)"); break; }
                t_check = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (rc) break;
        if (stats && i == n - 1) g_svc_ns_wait += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_sub).count();
        const uint32_t* rec = S->out + (size_t)k * kSvcOutDwords;
        uint8_t okv = rec[0] ? 1 : 0;
        int32_t nout = (int32_t)rec[5];
        int32_t stg = (int32_t)rec[1];
        if (okv && nout > m) { okv = 0; stg = 100; }  // refined list longer than the caller's row
        b->ok[i] = okv;
        if (okv) {
            memcpy(b->center + 4 * i, rec + 8, 16);
            memcpy(b->normal + 4 * i, rec + 12, 16);
            b->n_images[i] = nout;
            for (int q = 0; q < m; q++) b->images[(size_t)i * m + q] = q < nout ? (int32_t)rec[32 + q] : b->images[(size_t)i * m + q];
            if (b->color) memcpy(b->color + 3 * i, rec + 16, 12);
            if (b->ncc) memcpy(b->ncc + i, rec + 19, 4);
        }
        if (b->fmin) memcpy(b->fmin + i, rec + 20, 8);
        if (b->x) memcpy(b->x + 3 * i, rec + 22, 24);
        if (b->result) b->result[i] = (int32_t)rec[2];
        if (b->nevals) b->nevals[i] = (int32_t)rec[3];
        if (b->stage) b->stage[i] = stg;
        if (b->ngrabs) b->ngrabs[i] = (int32_t)rec[4];
    }
    if (stats) {
        const auto t_out = std::chrono::steady_clock::now();
        g_svc_calls++;
        g_svc_ns_lock += std::chrono::duration_cast<std::chrono::nanoseconds>(t_sub - t_in).count();
        g_svc_ns_total += std::chrono::duration_cast<std::chrono::nanoseconds>(t_out - t_in).count();
    }
    if (S->outstanding.fetch_sub(n, std::memory_order_acq_rel) == n) {  // I was the last one waiting
        std::lock_guard<std::mutex> lk(s->svc_mu);
        // nobody is waiting: let the launch end -- the one I published into (the object may have been reopened since:
        // a thread spinning in service_open goes on as soon as the count reaches zero)
        if (S->gen == my_gen && S->outstanding.load() == 0) service_close(*S);
    }
    return rc;
}

static int optimize_small_host_batch(const hpmvs_scene* s, const hpmvs_options* o, hpmvs_patch_batch* b) {
    const size_t n = (size_t)b->n, m = (size_t)b->max_images;
    const PoolLayout L = pool_layout(n, m);
    hpmvs_scene::StageEntry& e = s->stage[s->stage_next.fetch_add(1) % hpmvs_scene::kStageEntries];
    std::lock_guard<std::mutex> use(e.mu);
    if (!e.st || !e.dev || !e.host) {
        // all three or nothing: a failed allocation must not leave a half-initialised entry behind
        const PoolLayout cap = pool_layout((size_t)hpmvs_scene::kStageCapPatches, (size_t)HPMVS_MAX_IMAGES);
        Exclusive ex(s);  // (allocations wait for an idle device)
        hipStream_t st = e.st;
        char *dv = nullptr, *hv = nullptr;
        bool good = st || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
        good = good && hipMalloc((void**)&dv, cap.total) == hipSuccess;
        good = good && hipHostMalloc((void**)&hv, cap.total) == hipSuccess;
        if (!good) {
            if (dv) hipFree(dv);
            if (hv) hipHostFree(hv);
            if (st && !e.st) hipStreamDestroy(st);
            return fail(HPMVS_ERR_HIP, "optimize_batch: cannot allocate the staging block of a small host batch");
        }
        e.st = st; e.dev = dv; e.host = hv;
    }
    char* h = e.host;
    memcpy(h + L.off_center, b->center, 16 * n); memcpy(h + L.off_normal, b->normal, 16 * n);
    memcpy(h + L.off_scale, b->scale, 4 * n); memcpy(h + L.off_nimg, b->n_images, 4 * n);
    memcpy(h + L.off_images, b->images, 4 * n * m);
    HIPCHK(hipMemcpyAsync(e.dev, h, L.in_bytes, hipMemcpyHostToDevice, e.st));
    HIPCHK(hipMemsetAsync(e.dev + L.in_bytes, 0, L.total - L.in_bytes, e.st));
    DevBatch D;
    memset(&D, 0, sizeof(D));
    D.n = b->n; D.max_images = b->max_images;
    char* d = e.dev;
    D.center = (float*)(d + L.off_center); D.normal = (float*)(d + L.off_normal); D.scale = (float*)(d + L.off_scale);
    D.n_images = (int32_t*)(d + L.off_nimg); D.images = (int32_t*)(d + L.off_images);
    D.ok = (uint8_t*)(d + L.off_ok); D.color = (float*)(d + L.off_color); D.ncc = (float*)(d + L.off_ncc);
    D.fmin = (double*)(d + L.off_fmin); D.x = (double*)(d + L.off_x); D.result = (int32_t*)(d + L.off_result);
    D.nevals = (int32_t*)(d + L.off_nevals); D.stage = (int32_t*)(d + L.off_stage); D.ngrabs = (int32_t*)(d + L.off_ngrabs);
    const DevOptions dopt = make_dev_options(o);
    int rc;
    {
        std::lock_guard<std::recursive_mutex> lk(s->mu);
        if ((rc = enqueue_refinement(s, dopt, D, e.st))) return rc;
    }
    HIPCHK(hipMemcpyAsync(h, e.dev, L.total, hipMemcpyDeviceToHost, e.st));  // inputs come back refined in place
    HIPCHK(hipStreamSynchronize(e.st));
    memcpy(b->center, h + L.off_center, 16 * n); memcpy(b->normal, h + L.off_normal, 16 * n);
    memcpy(b->n_images, h + L.off_nimg, 4 * n); memcpy(b->images, h + L.off_images, 4 * n * m);
    memcpy(b->ok, h + L.off_ok, n);
    if (b->color) memcpy(b->color, h + L.off_color, 12 * n);
    if (b->ncc) memcpy(b->ncc, h + L.off_ncc, 4 * n);
    if (b->fmin) memcpy(b->fmin, h + L.off_fmin, 8 * n);
    if (b->x) memcpy(b->x, h + L.off_x, 24 * n);
    if (b->result) memcpy(b->result, h + L.off_result, 4 * n);
    if (b->nevals) memcpy(b->nevals, h + L.off_nevals, 4 * n);
    if (b->stage) memcpy(b->stage, h + L.off_stage, 4 * n);
    if (b->ngrabs) memcpy(b->ngrabs, h + L.off_ngrabs, 4 * n);
    return HPMVS_OK;
}

extern "C" {

int hpmvs_optimize_batch(const hpmvs_scene* s, const hpmvs_options* o, hpmvs_patch_batch* b, int on_device,
                         void* stream) {
    int rc = check_batch(s, o, b);
    if (rc) return rc;
    if (!b->ok) return fail(HPMVS_ERR_ARG, "optimize_batch: ok[] is required");
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    if (!on_device && !stream && b->n <= kServiceMaxPatches && b->max_images <= HPMVS_FAST_IMAGES && service_enabled()) {
        // The open batch runs the 64-id kernel alone.  A patch that comes back with stage 100 (its list outgrew 64 ids, or the
        // caller's row) was left untouched: it goes through a batch launch of its own, whose wide kernel takes lists up to
        // HPMVS_MAX_IMAGES (kernel_wide.hip) -- same result as if it had been part of a batch.
        std::vector<int32_t> stage_tmp;
        hpmvs_patch_batch bb = *b;
        if (!bb.stage) { stage_tmp.assign((size_t)b->n, 0); bb.stage = stage_tmp.data(); }
        if ((rc = optimize_through_service(s, o, &bb))) return rc;
        for (int i = 0; i < b->n; i++) {
            if (bb.ok[i] || bb.stage[i] != 100) continue;
            hpmvs_patch_batch one = bb;
            one.n = 1;
            one.center += 4 * i; one.normal += 4 * i; one.scale += i; one.n_images += i; one.images += (size_t)i * b->max_images; one.ok += i;
            if (one.color) one.color += 3 * i;
            if (one.ncc) one.ncc += i;
            if (one.fmin) one.fmin += i;
            if (one.x) one.x += 3 * i;
            if (one.result) one.result += i;
            if (one.nevals) one.nevals += i;
            if (one.stage) one.stage += i;
            if (one.ngrabs) one.ngrabs += i;
            if ((rc = optimize_small_host_batch(s, o, &one))) return rc;
        }
        return HPMVS_OK;
    }
    if (!on_device && !stream && b->n <= hpmvs_scene::kStageCapPatches) return optimize_small_host_batch(s, o, b);
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const DevBatch D = c.batch(b, Call::kRefine);
    if (!on_device) { s->last_staged_bytes = c.staged_bytes; s->last_mapped_bytes = c.mapped_bytes; }  // (hpmvs_last_staging)
    if ((rc = c.begin(st))) return rc;
    const DevOptions d = make_dev_options(o);
    {
        std::lock_guard<std::recursive_mutex> lk(s->mu);  // workspace hand-out + the scene's single event pair
        if ((rc = enqueue_refinement(s, d, D, st))) return rc;
    }
    return c.finish();
}

int hpmvs_init_patches_batch(const hpmvs_scene* s, const hpmvs_options* o, int start_level, int n_points,
                             const double* xyz, const int32_t* meas_off, const int32_t* meas_img, hpmvs_patch_batch* b,
                             int on_device, void* stream) {
    return hpmvs_init_patches_sphere_batch(s, o, start_level, n_points, xyz, meas_off, meas_img, nullptr, b, on_device, stream);
}

int hpmvs_init_patches_sphere_batch(const hpmvs_scene* s, const hpmvs_options* o, int start_level, int n_points,
                                    const double* xyz, const int32_t* meas_off, const int32_t* meas_img,
                                    const double* sphere, hpmvs_patch_batch* b, int on_device, void* stream) {
    int rc = check_batch_shape(s, o, b);
    if (rc) return rc;
    SeedSphere sph = {{0.0, 0.0, 0.0}, 0.0, 0};
    if (sphere) {
        // a centre that is not finite, a NaN or a negative radius: no sphere at all (r = +inf is one, and gates nothing)
        if (!std::isfinite(sphere[0]) || !std::isfinite(sphere[1]) || !std::isfinite(sphere[2]) || !(sphere[3] >= 0.0))
            return fail(HPMVS_ERR_ARG, "init_patches_batch: sphere needs a finite centre and a radius >= 0");
        sph.c[0] = sphere[0]; sph.c[1] = sphere[1]; sph.c[2] = sphere[2]; sph.r = sphere[3]; sph.on = 1;
    }
    if (b->n != n_points) return fail(HPMVS_ERR_ARG, "init_patches_batch: b->n must equal n_points");
    if (n_points > 0 && (!xyz || !meas_off || !b->center || !b->normal || !b->scale || !b->n_images ||
                         !b->images || !b->ok))
        return fail(HPMVS_ERR_ARG, "init_patches_batch: missing array");
    // meas_img may be NULL when no point has a measurement (every seed then fails with stage 10, like the
    // reference's empty image list); with host arrays that is checkable here
    if (n_points > 0 && !meas_img && (on_device || meas_off[n_points] != 0))
        return fail(HPMVS_ERR_ARG, "init_patches_batch: meas_img missing");
    if (start_level < 0 || start_level > o->MAXLEVEL) return fail(HPMVS_ERR_ARG, "init_patches_batch: bad start_level");
    if (n_points == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const DevBatch D = c.batch(b, Call::kCreate);
    // host arrays without any measurement: a one-element zero list (device pointers are handed through whatever the count)
    const size_t n = (size_t)n_points, nm = on_device ? 0 : (size_t)meas_off[n_points];
    const double* dxyz = c.in(xyz, 3 * n);
    const int32_t* doff = c.in(meas_off, n + 1);
    const int32_t* dimg = c.arr(meas_img, nm ? nm : 1, nm ? Call::kCopyIn : Call::kZero);
    if ((rc = c.begin())) return rc;
    const DevOptions d = make_dev_options(o);
    {
        std::lock_guard<std::recursive_mutex> lk(s->mu);
        launch_seed_init(dev_scene(s), d, start_level, n_points, dxyz, doff, dimg, sph, D, st);
        HIPCHK(hipGetLastError());
        if ((rc = enqueue_refinement(s, d, D, st))) return rc;
        launch_drift_gate(n_points, dxyz, D, st);
        HIPCHK(hipGetLastError());
    }
    return c.finish();
}

int hpmvs_expand_directions(int mode, float* dxdy) {
    if ((mode != HPMVS_EXPAND_EXTEND && mode != HPMVS_EXPAND_BRANCH) || !dxdy) return fail(HPMVS_ERR_ARG, "expand_directions: bad mode/pointer");
    const int N = expand_fanout(mode);
    for (int k = 0; k < 2 * N; k++) dxdy[k] = expand_direction_table(mode)[k];
    return N;
}

int hpmvs_expand_batch(const hpmvs_scene* s, const hpmvs_options* o, int mode, const hpmvs_patch_batch* parents,
                       const float* cell_center, const float* cell_width, const uint8_t* skip, hpmvs_patch_batch* out,
                       int on_device, void* stream) {
    if (mode != HPMVS_EXPAND_EXTEND && mode != HPMVS_EXPAND_BRANCH) return fail(HPMVS_ERR_ARG, "expand_batch: bad mode");
    int rc = check_batch(s, o, parents);
    if (rc) return rc;
    if ((rc = check_batch_shape(s, o, out))) return rc;
    const int N = expand_fanout(mode);
    if (out->n != parents->n * N) return fail(HPMVS_ERR_ARG, "expand_batch: out->n must be parents->n * fan-out");
    if (out->max_images != parents->max_images) return fail(HPMVS_ERR_ARG, "expand_batch: max_images mismatch");
    if (parents->n > 0 && (!cell_center || !cell_width || !out->center || !out->normal || !out->scale || !out->n_images ||
                           !out->images || !out->ok))
        return fail(HPMVS_ERR_ARG, "expand_batch: missing array");
    if (parents->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const size_t n = (size_t)parents->n;
    const DevBatch P = c.batch(parents, Call::kRead), D = c.batch(out, Call::kCreate);
    const float *dcc = c.in(cell_center, 3 * n), *dcw = c.in(cell_width, n);
    const uint8_t* dskip = c.in(skip, n * N);
    if ((rc = c.begin())) return rc;
    const DevOptions d = make_dev_options(o);
    {
        std::lock_guard<std::recursive_mutex> lk(s->mu);
        launch_expand_init(dev_scene(s), mode, parents->n, P, dcc, dcw, dskip, D, st);
        HIPCHK(hipGetLastError());
        if ((rc = enqueue_refinement(s, d, D, st))) return rc;
        launch_expand_gate(mode, parents->n, P, dcc, dcw, D, st);
        HIPCHK(hipGetLastError());
    }
    return c.finish();
}

// hpmvs_objective_batch is answered by the refinement kernel's own evaluator driven stand-alone (kernels_basic.hip).  A
// measurement build (`make LANE=1`, tools/objective_ab.py) also carries the one-lane-per-grab kernel of
// kernel_objective_lane.hip and runs it with HPMVS_OBJECTIVE_KERNEL=lane: same values, no faster (profiles/r05/lane_per_grab.txt).
static void launch_objective_chosen(const DevScene& sc, const DevOptions& d, const DevBatch& b, const double* x, double* f,
                                    int32_t* g, hipStream_t st) {
#ifdef HPMVS_WITH_LANE_KERNEL
    const char* e = getenv("HPMVS_OBJECTIVE_KERNEL");
    if (e && strcmp(e, "lane") == 0) { launch_objective_lane(sc, d, b, x, f, g, st); return; }
#endif
    launch_objective(sc, d, b, x, f, g, st);
}

int hpmvs_objective_batch(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* b, const double* x,
                          double* f_out, int32_t* ngrabs_out, int on_device, void* stream) {
    int rc = check_batch(s, o, b);
    if (rc) return rc;
    if (!x || !f_out) return fail(HPMVS_ERR_ARG, "objective_batch: x/f_out missing");
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const size_t n = (size_t)b->n;
    const DevBatch D = c.batch(b, Call::kRead);
    const double* dx = c.in(x, 3 * n);
    double* df = c.out(f_out, n);
    int32_t* dg = c.out(ngrabs_out, n);
    if ((rc = c.begin())) return rc;
    launch_objective_chosen(dev_scene(s), make_dev_options(o), D, dx, df, dg, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}

int hpmvs_inccs_batch(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* b, int ref_idx, int robust,
                      float* out, int on_device, void* stream) {
    int rc = check_batch(s, o, b);
    if (rc) return rc;
    if (!out || ref_idx < 0) return fail(HPMVS_ERR_ARG, "inccs_batch: out/ref_idx");
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const DevBatch D = c.batch(b, Call::kRead);
    float* dout = c.out(out, (size_t)b->n * b->max_images);
    if ((rc = c.begin())) return rc;
    launch_inccs(dev_scene(s), make_dev_options(o), D, ref_idx, robust, dout, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}

// ---- depth maps and the acceptance gates over them (kernel_depth.hip)
int hpmvs_scene_depth_reset(hpmvs_scene* s) {
    if (!s || !s->committed) return fail(HPMVS_ERR_STATE, "scene_depth_reset: scene not committed");
    HIPCHK(hipSetDevice(s->device));
    Exclusive ex(s);  // (the first call allocates: hipMalloc waits for an idle device, see Exclusive)
    if (!s->depth_pool || !s->ddepth) {
        // Scene.cpp:74-80: rows = height(level) / DEPTH_SUBSAMPLE, cols = width(level) / DEPTH_SUBSAMPLE (a double 2)
        size_t total = 0;
        std::vector<DevDepthView> hd((size_t)s->n_views, DevDepthView{});
        for (int v = 0; v < s->n_views; v++)
            for (int l = 0; l < s->hviews[v].n_levels; l++) {
                hd[v].rows[l] = (int)((double)s->hviews[v].h[l] / 2.0);
                hd[v].cols[l] = (int)((double)s->hviews[v].w[l] / 2.0);
                total += (size_t)hd[v].rows[l] * hd[v].cols[l];
            }
        if (total == 0) return fail(HPMVS_ERR_STATE, "scene_depth_reset: empty scene");
        // both buffers into locals; the scene sees them only when everything succeeded (a failure half way must not
        // leave a pool without its table: the kernels test one and dereference the other)
        float* pool = nullptr;
        DevDepthView* table = nullptr;
        struct Undo { float*& a; DevDepthView*& b; ~Undo() { if (a) hipFree(a); if (b) hipFree(b); } } undo{pool, table};
        HIPCHK(hipMalloc((void**)&pool, total * sizeof(float)));
        size_t off = 0;
        for (int v = 0; v < s->n_views; v++)
            for (int l = 0; l < s->hviews[v].n_levels; l++) {
                hd[v].d[l] = pool + off;
                off += (size_t)hd[v].rows[l] * hd[v].cols[l];
            }
        HIPCHK(hipMalloc((void**)&table, sizeof(DevDepthView) * (size_t)s->n_views));
        HIPCHK(hipMemcpy(table, hd.data(), sizeof(DevDepthView) * (size_t)s->n_views, hipMemcpyHostToDevice));
        if (s->depth_pool) hipFree(s->depth_pool);  // (a half-initialised scene of an older library state)
        if (s->ddepth) hipFree(s->ddepth);
        s->depth_pool = pool; s->ddepth = table; s->depth_floats = total; s->hdepth.swap(hd);
        s->bytes += total * sizeof(float) + sizeof(DevDepthView) * (size_t)s->n_views;
        pool = nullptr; table = nullptr;
    }
    launch_depth_fill(s->depth_pool, s->depth_floats, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));  // (not the whole device: an open batch of single-patch calls may be running)
    return HPMVS_OK;
}

static int depth_level(const hpmvs_scene* s, int view, int level, const char* who, float** p, int* rows, int* cols) {
    if (!s || !s->depth_pool || !s->ddepth) return fail(HPMVS_ERR_STATE, std::string(who) + ": call hpmvs_scene_depth_reset first");
    if (view < 0 || view >= s->n_views || level < 0 || level >= s->hviews[view].n_levels)
        return fail(HPMVS_ERR_ARG, std::string(who) + ": bad view / level");
    *p = s->hdepth[view].d[level]; *rows = s->hdepth[view].rows[level]; *cols = s->hdepth[view].cols[level];
    return HPMVS_OK;
}
}  // extern "C"
// (capi_common.hpp: the depth-image entries of capi_image.hip)
int hpmvs::capi::scene_depth_maps(const hpmvs_scene* s, int view, int level, const char* who, SceneDepthMaps* out) {
    float* p; int r, c, rc;
    if ((rc = depth_level(s, view, level == HPMVS_DEPTH_COMBINED ? 0 : level, who, &p, &r, &c))) return rc;
    out->device = s->device;
    out->n_levels = s->hviews[view].n_levels;
    out->maps = s->hdepth[view];
    return HPMVS_OK;
}
extern "C" {
int hpmvs_scene_depth_set_level(hpmvs_scene* s, int view, int level, const float* data, int rows, int cols) {
    float* p; int r, c, rc;
    if ((rc = depth_level(s, view, level, "scene_depth_set_level", &p, &r, &c))) return rc;
    if (!data || rows != r || cols != c) return fail(HPMVS_ERR_ARG, "scene_depth_set_level: shape is not rows x cols of that level");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpy(p, data, sizeof(float) * (size_t)r * c, hipMemcpyHostToDevice));
    return HPMVS_OK;
}
int hpmvs_scene_depth_get_level(const hpmvs_scene* s, int view, int level, float* data, size_t capacity, int* rows, int* cols) {
    float* p; int r, c, rc;
    if ((rc = depth_level(s, view, level, "scene_depth_get_level", &p, &r, &c))) return rc;
    if (rows) *rows = r;
    if (cols) *cols = c;
    if (!data) return HPMVS_OK;  // shape query
    if (capacity < (size_t)r * c) return fail(HPMVS_ERR_ARG, "scene_depth_get_level: buffer too small");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(data, p, sizeof(float) * (size_t)r * c, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

static int check_depth_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, const char* who) {
    if (!s || !b) return fail(HPMVS_ERR_ARG, std::string(who) + ": null scene / batch");
    if (!s->committed || !s->depth_pool || !s->ddepth) return fail(HPMVS_ERR_STATE, std::string(who) + ": call hpmvs_scene_depth_reset first");
    if (b->n < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, std::string(who) + ": bad n/max_images");
    if (b->n > 0 && (!b->center || !b->normal || !b->scale || !b->n_images || !b->images))
        return fail(HPMVS_ERR_ARG, std::string(who) + ": batch input arrays missing");
    return HPMVS_OK;
}
int hpmvs_set_depths_batch(hpmvs_scene* s, const hpmvs_patch_batch* b, int on_device, void* stream) {
    int rc = check_depth_batch(s, b, "set_depths_batch");
    if (rc) return rc;
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    DevBatch D = c.batch(b, Call::kRead);
    D.ok = c.in(b->ok, (size_t)b->n);  // optional: without it every patch counts
    if ((rc = c.begin())) return rc;
    launch_set_depths(dev_scene(s), s->ddepth, D, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}
// Scene::setDepths(patch_i, subtract[i]) for i = 0 .. n - 1 IN THAT ORDER (kernel_depth.hip: keys, sort, per-cell replay).
// Without a subtraction the calls commute and the batch goes to set_depths_kernel.
int hpmvs_depth_ops_batch(hpmvs_scene* s, const hpmvs_patch_batch* b, const uint8_t* subtract, int on_device, void* stream) {
    int rc = check_depth_batch(s, b, "depth_ops_batch");
    if (rc) return rc;
    if (b->n == 0) return HPMVS_OK;
    if (!subtract) return hpmvs_set_depths_batch(s, b, on_device, stream);
    const size_t cap = (size_t)b->n * (size_t)b->max_images;
    if (cap >= ((size_t)1 << 28)) return fail(HPMVS_ERR_ARG, "depth_ops_batch: n * max_images must stay below 2^28 (apply the level in pieces: the order between pieces is kept)");
    if (s->depth_floats >= ((size_t)1 << 32)) return fail(HPMVS_ERR_STATE, "depth_ops_batch: the scene's depth maps hold 2^32 cells or more");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    DevBatch D = c.batch(b, Call::kRead);
    D.ok = c.in(b->ok, (size_t)b->n);
    const uint8_t* dsub = c.in(subtract, (size_t)b->n);
    unsigned long long* keys = (unsigned long long*)c.scratch(cap * sizeof(unsigned long long));
    unsigned long long* sorted = (unsigned long long*)c.scratch(cap * sizeof(unsigned long long));
    unsigned int* counter = (unsigned int*)c.scratch(sizeof(unsigned int));
    if ((rc = c.begin())) return rc;
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned int), st));
    launch_depth_ops_keys(dev_scene(s), s->ddepth, s->depth_pool, D, keys, counter, st);
    HIPCHK(hipGetLastError());
    unsigned int count = 0;  // the sort's size depends on it: read back mid-call
    HIPCHK(hipMemcpyAsync(&count, counter, sizeof(count), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (count == 0) return HPMVS_OK;
    size_t temp_bytes = 0;
    if (depth_ops_sort(nullptr, &temp_bytes, keys, sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, "depth_ops_batch: rocPRIM size query failed");
    void* temp = c.scratch(temp_bytes ? temp_bytes : 1);
    if (!temp) return c.error();
    if (depth_ops_sort(temp, &temp_bytes, keys, sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, "depth_ops_batch: rocPRIM sort failed");
    launch_depth_ops_apply(dev_scene(s), s->ddepth, s->depth_pool, D, dsub, sorted, count, st);
    HIPCHK(hipGetLastError());
    return c.finish();  // (waits in both forms: the temporaries are freed when this call returns)
}
// Scene::getLevelSupport(patch, minLevel) (src/hpmvs/Scene.cpp:334-343) per patch
int hpmvs_level_support_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, int min_level, int32_t* support, int on_device, void* stream) {
    if (!s || !b || !support) return fail(HPMVS_ERR_ARG, "level_support_batch: null argument");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "level_support_batch: scene not committed");
    if (b->n < 0 || b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, "level_support_batch: bad n/max_images");
    if (b->n > 0 && (!b->center || !b->scale || !b->n_images || !b->images)) return fail(HPMVS_ERR_ARG, "level_support_batch: batch input arrays missing");
    if (b->n == 0) return HPMVS_OK;
    int rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const DevBatch D = c.batch(b, Call::kRead);
    int32_t* dsup = c.out(support, (size_t)b->n);
    if ((rc = c.begin())) return rc;
    launch_level_support(dev_scene(s), D, min_level, dsup, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}
// CellProcessor::regularize (src/hpmvs/CellProcessor.cpp:309-367) for a level of cells against a versioned leaf table
// (kernel_regularize.hip).  Every device byte comes from a launch workspace: [1 KB counter block, untouched] [header] [hash keys]
// [hash values] and, for host pointers, the leaf table and the cells in chunks that fit the rest.  The scene lock is held for the
// whole call (the workspace is this call's until its last kernel has been enqueued).
int hpmvs_regularize_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, const float* cell_width, const int32_t* position,
                           const uint8_t* expanded, const hpmvs_leaf_table* lt, float* flatness, int32_t* n_neighbours,
                           int32_t* neighbour_leaf, int on_device, void* stream) {
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, "regularize_batch: no HIP device visible");
    if (!s || !b || !lt) return fail(HPMVS_ERR_ARG, "regularize_batch: null scene / cells / leaf table");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "regularize_batch: scene not committed");
    if (b->n < 0 || lt->n < 0) return fail(HPMVS_ERR_ARG, "regularize_batch: negative count");
    if (b->n > 0 && (b->max_images < 1 || !b->center || !b->normal || !b->n_images || !b->images || !cell_width || !position ||
                     !expanded || !flatness || !n_neighbours))
        return fail(HPMVS_ERR_ARG, "regularize_batch: cell arrays missing");
    if (lt->n > 0 && (!lt->cell_center || !lt->cell_width || !lt->patch_center || !lt->born || !lt->died))
        return fail(HPMVS_ERR_ARG, "regularize_batch: leaf table arrays missing");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(lt->root_center[k])) return fail(HPMVS_ERR_ARG, "regularize_batch: root centre not finite");
    if (!(lt->root_width > 0.0f) || !std::isfinite(lt->root_width)) return fail(HPMVS_ERR_ARG, "regularize_batch: root width must be finite and > 0");
    if (b->n == 0) return HPMVS_OK;
    const size_t n = (size_t)b->n, L = (size_t)lt->n;
    std::vector<int32_t> href;
    if (!on_device) {   // the reference image of an expanded cell must be a view of the scene (host arrays: checked here)
        href.resize(n);
        for (size_t i = 0; i < n; i++) {
            href[i] = b->images[i * (size_t)b->max_images];
            if (expanded[i] && (b->n_images[i] < 1 || href[i] < 0 || href[i] >= s->n_views))
                return fail(HPMVS_ERR_ARG, "regularize_batch: an expanded cell's reference image is not a view of the scene");
        }
    }
    size_t slots = 2;
    while (slots < 2 * L) slots <<= 1;
    const size_t o_hdr = kQueueSlotBytes, o_keys = reg_align(o_hdr + 16), o_vals = reg_align(o_keys + 8 * slots);
    size_t o_end = reg_align(o_vals + 4 * slots);
    size_t o_lcc = 0, o_lcw = 0, o_lpc = 0, o_lb = 0, o_ld = 0;
    if (!on_device) {
        o_lcc = o_end; o_lcw = reg_align(o_lcc + 12 * L); o_lpc = reg_align(o_lcw + 4 * L); o_lb = reg_align(o_lpc + 12 * L);
        o_ld = reg_align(o_lb + 4 * L); o_end = reg_align(o_ld + 4 * L);
    }
    // host cells: 16 + 16 (centre, normal) + 4 x 4 (ref, width, position, flatness) + 1 (expanded) + 4 + 96 (outputs) bytes, 8 arrays
    const size_t per_cell = 149, chunk_min = 1024;
    if (slots > ((size_t)1 << 30) || o_end + (on_device ? 0 : chunk_min * per_cell + 8 * 256) > s->ws_bytes)
        return fail(HPMVS_ERR_ARG, "regularize_batch: the leaf table does not fit the launch workspace");
    int rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> lk(s->mu);
    if ((rc = service_quiesce(s))) return rc;
    Workspace ws(s, st);
    if (ws.rc) return ws.rc;
    char* w = (char*)ws.q;
    int32_t* hdr = (int32_t*)(w + o_hdr);
    RegTree t;
    t.root[0] = lt->root_center[0]; t.root[1] = lt->root_center[1]; t.root[2] = lt->root_center[2]; t.root[3] = lt->root_width;
    t.n = lt->n; t.slots = (int32_t)slots;
    t.keys = (unsigned long long*)(w + o_keys); t.vals = (int32_t*)(w + o_vals);
    if (on_device) {
        t.cell_center = lt->cell_center; t.cell_width = lt->cell_width; t.patch_center = lt->patch_center; t.born = lt->born; t.died = lt->died;
    } else {
        t.cell_center = (const float*)(w + o_lcc); t.cell_width = (const float*)(w + o_lcw); t.patch_center = (const float*)(w + o_lpc);
        t.born = (const int32_t*)(w + o_lb); t.died = (const int32_t*)(w + o_ld);
        if (L) {
            HIPCHK(hipMemcpyAsync((void*)t.cell_center, lt->cell_center, 12 * L, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync((void*)t.cell_width, lt->cell_width, 4 * L, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync((void*)t.patch_center, lt->patch_center, 12 * L, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync((void*)t.born, lt->born, 4 * L, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync((void*)t.died, lt->died, 4 * L, hipMemcpyHostToDevice, st));
        }
    }
    HIPCHK(hipMemsetAsync(hdr, 0, 16, st));
    HIPCHK(hipMemsetAsync(t.keys, 0, 8 * slots, st));
    launch_regularize_leaves(t, on_device ? b->n : 0, s->n_views, b->images, b->max_images, b->n_images, expanded, hdr, st);
    HIPCHK(hipGetLastError());
    int32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[0] & 1) return fail(HPMVS_ERR_ARG, "regularize_batch: a leaf's centre is not the one the root's subdivision gives for its width, or it lies deeper than 21 levels");
    if (h[0] & 2) return fail(HPMVS_ERR_ARG, "regularize_batch: an expanded cell's reference image is not a view of the scene");
    const int max_depth = h[1], min_depth = kRegMaxDepth + 1 - h[2];
    const DevScene sc = dev_scene(s);
    RegCells cl;
    if (on_device) {
        cl.n = b->n; cl.ref_stride = b->max_images;
        cl.center = b->center; cl.normal = b->normal; cl.ref = b->images; cl.width = cell_width; cl.position = position; cl.expanded = expanded;
        cl.flatness = flatness; cl.n_neighbours = n_neighbours; cl.neighbour = neighbour_leaf;
        launch_regularize(sc, t, cl, min_depth, max_depth, st);
        HIPCHK(hipGetLastError());
        return HPMVS_OK;
    }
    const size_t chunk = std::min(n, (s->ws_bytes - o_end - 8 * 256) / per_cell);
    char* c0 = w + o_end;
    float* dcen = (float*)c0;
    float* dnor = (float*)(c0 + reg_align(16 * chunk));
    int32_t* dref = (int32_t*)((char*)dnor + reg_align(16 * chunk));
    float* dwid = (float*)((char*)dref + reg_align(4 * chunk));
    int32_t* dpos = (int32_t*)((char*)dwid + reg_align(4 * chunk));
    float* dfl = (float*)((char*)dpos + reg_align(4 * chunk));
    int32_t* dnn = (int32_t*)((char*)dfl + reg_align(4 * chunk));
    int32_t* dnb = (int32_t*)((char*)dnn + reg_align(4 * chunk));
    uint8_t* dexp = (uint8_t*)((char*)dnb + reg_align(96 * chunk));
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        HIPCHK(hipMemcpyAsync(dcen, b->center + 4 * i0, 16 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dnor, b->normal + 4 * i0, 16 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dref, href.data() + i0, 4 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dwid, cell_width + i0, 4 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dpos, position + i0, 4 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dfl, flatness + i0, 4 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dexp, expanded + i0, m, hipMemcpyHostToDevice, st));
        cl.n = (int32_t)m; cl.ref_stride = 1;
        cl.center = dcen; cl.normal = dnor; cl.ref = dref; cl.width = dwid; cl.position = dpos; cl.expanded = dexp;
        cl.flatness = dfl; cl.n_neighbours = dnn; cl.neighbour = neighbour_leaf ? dnb : nullptr;
        launch_regularize(sc, t, cl, min_depth, max_depth, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(flatness + i0, dfl, 4 * m, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(n_neighbours + i0, dnn, 4 * m, hipMemcpyDeviceToHost, st));
        if (neighbour_leaf) HIPCHK(hipMemcpyAsync(neighbour_leaf + 24 * i0, dnb, 96 * m, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return HPMVS_OK;
}
// CellProcessor::filter (src/hpmvs/CellProcessor.cpp:43-82) for every cell of a level (kernel_filter.hip).  The offsets are
// validated before any output is written: on the host for host pointers, by filter_check_kernel (verdict read back) for device
// pointers.
int hpmvs_filter_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, const int32_t* cell_start, int n_cells, float* dist,
                       int32_t* keep, int on_device, void* stream) {
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, "filter_batch: no HIP device visible");
    if (!s || !b) return fail(HPMVS_ERR_ARG, "filter_batch: null scene / batch");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "filter_batch: scene not committed");
    if (b->n < 0 || n_cells < 0) return fail(HPMVS_ERR_ARG, "filter_batch: negative count");
    if (!cell_start) return fail(HPMVS_ERR_ARG, "filter_batch: cell_start missing");
    if (b->n > 0 && (!b->center || !b->normal || !dist)) return fail(HPMVS_ERR_ARG, "filter_batch: batch arrays missing");
    if (n_cells > 0 && !keep) return fail(HPMVS_ERR_ARG, "filter_batch: keep missing");
    static const char* kBadOffsets = "filter_batch: cell_start must start at 0, not decrease and end at the batch's row count";
    if (!on_device) {
        if (cell_start[0] != 0 || cell_start[n_cells] != b->n) return fail(HPMVS_ERR_ARG, kBadOffsets);
        for (int c = 0; c < n_cells; c++)
            if (cell_start[c + 1] < cell_start[c]) return fail(HPMVS_ERR_ARG, kBadOffsets);
    }
    if (b->n == 0 && n_cells == 0 && !on_device) return HPMVS_OK;
    int rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)b->n, nc = (size_t)n_cells;
    Call c(s, on_device, st);
    const float *dcen = c.in(b->center, 4 * n), *dnor = c.in(b->normal, 4 * n);
    const int32_t* dcs = c.in(cell_start, nc + 1);
    float* ddist = c.arr(dist, n, Call::kCopyBack);   // (the kernel writes every row and every cell: no zero fill)
    int32_t* dkeep = c.arr(keep, nc, Call::kCopyBack);
    int32_t* bad = on_device ? (int32_t*)c.scratch(sizeof(int32_t)) : nullptr;  // (host offsets were checked above)
    if ((rc = c.begin(st))) return rc;
    if (on_device) {
        int32_t h = 0;
        HIPCHK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
        launch_filter_check(dcs, n_cells, b->n, bad, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h) return fail(HPMVS_ERR_ARG, kBadOffsets);
    }
    launch_filter(dcen, dnor, dcs, n_cells, b->n, ddist, dkeep, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}
// The second half of Scene::initPatches (src/hpmvs/Scene.cpp:183-199) for the rows with ok != 0 (kernel_seed_tree.hip): bounding
// box, root, scale floor, the octree of the sequential patchTree_.add loop as leaf tables, and setDepths.  The root is known only
// on the device; a root that is not finite raises a flag there that every writing kernel honours, and the one read-back of the
// call's record (before setDepths is enqueued) turns it into the refusal.
static_assert(sizeof(hpmvs_seed_tree_info) == 28 && (kSeedBlkInts - kSeedBlkInfo) * 4 >= 28, "hpmvs_seed_tree_info is 7 words of the device record");
int hpmvs_seed_tree_batch(hpmvs_scene* s, hpmvs_patch_batch* b, int patch_init_maxlevel, int set_depths, hpmvs_seed_tree_info* info,
                          int32_t* rows, int32_t* cell_start, float* cell_center, float* cell_width, int32_t* cell_level,
                          float* patch_center, int on_device, void* stream) {
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, "seed_tree_batch: no HIP device visible");
    if (!s || !b || !info) return fail(HPMVS_ERR_ARG, "seed_tree_batch: null scene / batch / info");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "seed_tree_batch: scene not committed");
    if (b->n < 0) return fail(HPMVS_ERR_ARG, "seed_tree_batch: negative count");
    if (patch_init_maxlevel < 0 || patch_init_maxlevel > HPMVS_MAX_TREE_DEPTH)
        return fail(HPMVS_ERR_ARG, "seed_tree_batch: PATCH_INIT_MAXLEVEL must lie in 0 .. 21 (a deeper floor exceeds HPMVS_MAX_TREE_DEPTH)");
    if (!cell_start) return fail(HPMVS_ERR_ARG, "seed_tree_batch: cell_start missing");
    if (b->n > 0 && (!b->center || !b->scale || !rows || !cell_center || !cell_width || !cell_level))
        return fail(HPMVS_ERR_ARG, "seed_tree_batch: batch or output arrays missing");
    if (set_depths) {
        if (!s->depth_pool || !s->ddepth) return fail(HPMVS_ERR_ARG, "seed_tree_batch: set_depths on a scene without depth maps (hpmvs_scene_depth_reset)");
        if (b->n > 0 && (b->max_images < 1 || b->max_images > HPMVS_MAX_IMAGES || !b->normal || !b->n_images || !b->images))
            return fail(HPMVS_ERR_ARG, "seed_tree_batch: set_depths needs the batch's normals and image lists");
    }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (b->n == 0) {   // getBoundingBox's unit cube
        const seed::Root r = seed::make_root(nullptr, nullptr, 0, patch_init_maxlevel);
        if (on_device) HIPCHK(hipMemsetAsync(cell_start, 0, sizeof(int32_t), st));
        else cell_start[0] = 0;
        memcpy(info->root_center, r.c, sizeof(r.c));
        info->root_width = r.w; info->scale_floor = r.floor; info->n_rows = 0; info->n_leaves = 0;
        return HPMVS_OK;
    }
    int rc;
    const size_t n = (size_t)b->n;
    Call c(s, on_device, st);
    DevBatch D;
    memset(&D, 0, sizeof(D));
    D.n = b->n; D.max_images = b->max_images;
    D.center = c.in(b->center, 4 * n);
    D.scale = c.arr(b->scale, n, Call::kCopyIn | Call::kCopyBack);   // in/out: the floor
    D.ok = c.in(b->ok, n);                                            // optional: without it every row counts
    if (set_depths) {
        D.normal = c.in(b->normal, 4 * n);
        D.n_images = c.in(b->n_images, n);
        D.images = c.in(b->images, n * (size_t)b->max_images);
    }
    // (the emit kernel writes every entry of every output, zeros behind the counts, or nothing at all: no zero fill)
    SeedTreeOut out;
    out.rows = c.arr(rows, n, Call::kCopyBack);
    out.cell_start = c.arr(cell_start, n + 1, Call::kCopyBack);
    out.cell_center = c.arr(cell_center, 3 * n, Call::kCopyBack);
    out.cell_width = c.arr(cell_width, n, Call::kCopyBack);
    out.cell_level = c.arr(cell_level, n, Call::kCopyBack);
    out.patch_center = c.arr(patch_center, 3 * n, Call::kCopyBack);
    // the temporaries, O(n), as one block: 64 bytes per row and rocPRIM's own scratch (a function of n alone)
    SeedTreeScratch t;
    t.temp_bytes = seed_tree_temp_bytes(b->n);
    const size_t a8 = reg_align(8 * n), a4 = reg_align(4 * n), a0 = reg_align(sizeof(int32_t) * kSeedBlkInts);
    char* w = (char*)c.scratch(a0 + 5 * a8 + 4 * a4 + t.temp_bytes);
    t.blk = (int32_t*)w; w += a0;
    t.key_a = (unsigned long long*)w; w += a8;
    t.key_b = (unsigned long long*)w; w += a8;
    t.pair_a = (seed::Clamp*)w; w += a8;
    t.pair_b = (seed::Clamp*)w; w += a8;
    t.pair_c = (seed::Clamp*)w; w += a8;
    t.row_a = (int32_t*)w; w += a4;
    t.row_b = (int32_t*)w; w += a4;
    t.dep = (int32_t*)w; w += a4;
    t.depth = (int32_t*)w; w += a4;
    t.temp = w;
    if ((rc = c.begin(st))) return rc;
    if (launch_seed_tree(D.center, D.scale, D.ok, b->n, patch_init_maxlevel, t, out, st) != 0)
        return fail(HPMVS_ERR_HIP, "seed_tree_batch: a rocPRIM call failed");
    HIPCHK(hipGetLastError());
    int32_t h[kSeedBlkInts];
    HIPCHK(hipMemcpyAsync(h, t.blk, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[kSeedBlkBad]) return fail(HPMVS_ERR_ARG, "seed_tree_batch: the survivors' bounding box is not finite");
    memcpy(info, h + kSeedBlkInfo, sizeof(*info));
    if (set_depths) {
        launch_set_depths(dev_scene(s), s->ddepth, D, st);
        HIPCHK(hipGetLastError());
    }
    return c.finish();   // (waits in both forms: the temporaries are freed when this call returns)
}
// ---- the scheduler's octree as path keys (hpmvs_octree_index; kernel_octree.hip, kernel_octree_insert.hip, octree.hpp).  The
// look-up table lives in a launch workspace: [1 KB counter block, untouched] [verdict] [keys] [values]; the arrays go through
// Call.  The verdict of the check kernel is read back before the kernel that uses the table is enqueued: a refused table
// writes nothing.
struct OctreeLayout { size_t slots, o_hdr, o_keys, o_vals, bytes; };
// own: the table goes into a buffer of the call's own (L->bytes of it, no counter block ahead of the verdict) instead of a workspace
static int octree_index_check(const hpmvs_scene* s, const hpmvs_octree_index* t, int n, const float* points, const std::string& who,
                              OctreeLayout* L, bool own = false) {
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, who + ": no HIP device visible");
    if (!s || !t) return fail(HPMVS_ERR_ARG, who + ": null scene / octree");
    if (!s->committed) return fail(HPMVS_ERR_STATE, who + ": scene not committed");
    if (n < 0 || t->n_branches < 0 || t->n_leaves < 0) return fail(HPMVS_ERR_ARG, who + ": negative count");
    if ((t->n_branches > 0 && !t->branch_key) || (t->n_leaves > 0 && !t->leaf_key)) return fail(HPMVS_ERR_ARG, who + ": key arrays missing");
    if (n > 0 && !points) return fail(HPMVS_ERR_ARG, who + ": points missing");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(t->root_center[k])) return fail(HPMVS_ERR_ARG, who + ": root centre not finite");
    if (!(t->root_width > 0.0f) || !std::isfinite(t->root_width)) return fail(HPMVS_ERR_ARG, who + ": root width must be finite and > 0");
    const size_t nk = (size_t)t->n_branches + (size_t)t->n_leaves;
    if (nk > ((size_t)1 << 29)) return fail(HPMVS_ERR_ARG, who + ": the octree does not fit the launch workspace");
    L->slots = octree::table_slots(nk);
    L->o_hdr = own ? 0 : kQueueSlotBytes;
    L->o_keys = reg_align(L->o_hdr + 16);
    L->o_vals = reg_align(L->o_keys + 8 * L->slots);
    L->bytes = reg_align(L->o_vals + 4 * L->slots);
    if (!own && L->bytes > s->ws_bytes) return fail(HPMVS_ERR_ARG, who + ": the octree does not fit the launch workspace");
    return HPMVS_OK;
}
// builds and checks the table in the buffer w it is given, laid out by L (a workspace the caller holds, or memory of the call's
// own); host-synchronous up to the verdict
static int octree_table_build(const hpmvs_octree_index* t, const unsigned long long* dbk, const unsigned long long* dlk, const OctreeLayout& L,
                              char* w, hipStream_t st, const std::string& who) {
    int32_t* verdict = (int32_t*)(w + L.o_hdr);
    unsigned long long* keys = (unsigned long long*)(w + L.o_keys);
    int32_t* vals = (int32_t*)(w + L.o_vals);
    HIPCHK(hipMemsetAsync(verdict, 0, 16, st));
    HIPCHK(hipMemsetAsync(keys, 0, 8 * L.slots, st));
    if (t->n_branches + t->n_leaves == 0) return HPMVS_OK;
    launch_octree_build(dbk, t->n_branches, dlk, t->n_leaves, keys, vals, (uint32_t)L.slots, verdict, st);
    HIPCHK(hipGetLastError());
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, verdict, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h & octree::kBadKey) return fail(HPMVS_ERR_ARG, who + ": a word is no path key of a cell below the root (a leaf deeper than 21 levels, a branch deeper than 20)");
    if (h & octree::kBadTwice) return fail(HPMVS_ERR_ARG, who + ": a key occurs twice (within the branch or leaf keys, or in both)");
    if (h & octree::kBadOrphan) return fail(HPMVS_ERR_ARG, who + ": a key's parent prefix is neither a branch nor the root");
    return HPMVS_OK;
}
// The single tree's table in a launch workspace, for the rest of a call that declares it behind begin() (check rc): the scene lock
// is held from here to the call's return -- the workspace is the call's until its last kernel has been enqueued -- the open batches
// are drained and the table is built and verified.
struct WorkspaceTable {
    std::lock_guard<std::recursive_mutex> lk;
    std::optional<Workspace> ws;   // (behind lk: released before the lock is)
    const float root[4];
    unsigned long long* keys = nullptr;
    int32_t* vals = nullptr;
    const uint32_t slots;
    int rc;
    WorkspaceTable(const hpmvs_scene* s, const hpmvs_octree_index* t, const unsigned long long* dbk, const unsigned long long* dlk,
                   const OctreeLayout& L, hipStream_t st, const std::string& who)
        : lk(s->mu), root{t->root_center[0], t->root_center[1], t->root_center[2], t->root_width}, slots((uint32_t)L.slots) {
        if ((rc = service_quiesce(s))) return;
        ws.emplace(s, st);
        if ((rc = ws->rc)) return;
        char* w = (char*)ws->q;
        keys = (unsigned long long*)(w + L.o_keys); vals = (int32_t*)(w + L.o_vals);
        rc = octree_table_build(t, dbk, dlk, L, w, st, who);
    }
};
// root->at(p), Cell::contains and addConditional's target for a level's points against the scheduler's octree
int hpmvs_octree_locate_batch(const hpmvs_scene* s, const hpmvs_octree_index* t, int n, const float* points, const float* add_width,
                              uint8_t* inside, uint64_t* leaf_key, int32_t* leaf_index, float* leaf_width, float* leaf_center,
                              uint64_t* target_key, int on_device, void* stream) {
    const char* who = "octree_locate_batch";
    OctreeLayout L;
    int rc = octree_index_check(s, t, n, points, who, &L);
    if (rc) return rc;
    const size_t nb = (size_t)t->n_branches, nl = (size_t)t->n_leaves, np = (size_t)n;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const unsigned long long* dbk = (const unsigned long long*)c.in(t->branch_key, nb);
    const unsigned long long* dlk = (const unsigned long long*)c.in(t->leaf_key, nl);
    const float* dpts = c.in(points, 3 * np);
    const float* daw = c.in(add_width, np);
    OctreeLocateOut out;   // (the kernel writes every entry of every output it is given: no zero fill)
    out.inside = c.arr(inside, np, Call::kCopyBack);
    out.leaf_key = (unsigned long long*)c.arr(leaf_key, np, Call::kCopyBack);
    out.leaf_index = c.arr(leaf_index, np, Call::kCopyBack);
    out.leaf_width = c.arr(leaf_width, np, Call::kCopyBack);
    out.leaf_center = c.arr(leaf_center, 3 * np, Call::kCopyBack);
    out.target_key = (unsigned long long*)c.arr(target_key, np, Call::kCopyBack);
    if ((rc = c.begin(st))) return rc;
    WorkspaceTable tt(s, t, dbk, dlk, L, st, who);
    if (tt.rc) return tt.rc;
    launch_octree_locate(tt.root, tt.keys, tt.vals, tt.slots, n, dpts, daw, out, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}
// ---- what an extend level is whichever look-ups it makes (hpmvs_extend_tree_batch, hpmvs_extend_forest_batch): the shape of
// its candidates, the key arrays, and the enqueue order around the two look-up launches
static int extend_out_check(const std::string& who, const hpmvs_patch_batch* parents, const hpmvs_patch_batch* out) {
    if (out->n != parents->n * expand_fanout(HPMVS_EXPAND_EXTEND)) return fail(HPMVS_ERR_ARG, who + ": out->n must be 6 * parents->n");
    if (out->max_images != parents->max_images) return fail(HPMVS_ERR_ARG, who + ": max_images mismatch");
    if (parents->n > 0 && (!out->center || !out->normal || !out->scale || !out->n_images || !out->images || !out->ok))
        return fail(HPMVS_ERR_ARG, who + ": missing array");
    return HPMVS_OK;
}
static ExtendTreeOut extend_keys(Call& c, const hpmvs_extend_tree_keys* keys, size_t nc) {
    ExtendTreeOut K;
    memset(&K, 0, sizeof(K));
    if (keys) {   // (the two kernels write every entry of what they are given: no zero fill)
        K.skip = c.arr(keys->skip, nc, Call::kCopyBack);
        K.pre_inside = c.arr(keys->pre_inside, nc, Call::kCopyBack);
        K.pre_key = (unsigned long long*)c.arr(keys->pre_key, nc, Call::kCopyBack);
        K.border = c.arr(keys->border, nc, Call::kCopyBack);
        K.post_key = (unsigned long long*)c.arr(keys->post_key, nc, Call::kCopyBack);
    }
    return K;
}
// dcw: [parents->n], cell_width of expand_init / expand_gate: `width` for every parent (mode 0 reads no cell_center).  pre / post
// enqueue the look-ups before and after the refinement.
static int extend_enqueue(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* parents, const DevBatch& P, const DevBatch& D,
                          float width, float* dcw, hipStream_t st, const std::function<void()>& pre, const std::function<void()>& post) {
    const DevOptions d = make_dev_options(o);
    uint32_t wbits;
    memcpy(&wbits, &width, 4);
    int rc;
    std::lock_guard<std::recursive_mutex> lk(s->mu);
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dcw, (int)wbits, (size_t)parents->n, st));
    launch_expand_init(dev_scene(s), HPMVS_EXPAND_EXTEND, parents->n, P, nullptr, dcw, nullptr, D, st);
    HIPCHK(hipGetLastError());
    pre();
    HIPCHK(hipGetLastError());
    if ((rc = enqueue_refinement(s, d, D, st))) return rc;
    launch_expand_gate(HPMVS_EXPAND_EXTEND, parents->n, P, nullptr, dcw, D, st);
    HIPCHK(hipGetLastError());
    post();
    HIPCHK(hipGetLastError());
    return HPMVS_OK;
}
// One extend level's candidate steps against the real tree (CellProcessor.cpp:84-178; kernel_extend_tree.hip): expand_init, the pre
// look-up, the refinement, the gates, the post look-up.  The table is built once and must outlive the refinement launch, which
// takes a workspace itself (on one stream: the very one a look-up call would hold), so it lives in memory of this call's own.
// Two Calls: the keys and the table first, so that the table's verdict is in before a batch array is declared -- an output in
// pinned host memory is cleared in place by begin().
int hpmvs_extend_tree_batch(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_octree_index* t, const hpmvs_patch_batch* parents,
                            float width, hpmvs_patch_batch* out, const hpmvs_extend_tree_keys* keys, int on_device, void* stream) {
    const std::string who = "extend_tree_batch";
    int rc = check_batch(s, o, parents);
    if (rc) return rc;
    if ((rc = check_batch_shape(s, o, out))) return rc;
    OctreeLayout L;
    if ((rc = octree_index_check(s, t, 0, nullptr, who, &L, true))) return rc;
    if ((rc = extend_out_check(who, parents, out))) return rc;
    if (!std::isfinite(width) || octree::level_depth(t->root_width, width) < 0)
        return fail(HPMVS_ERR_ARG, who + ": width is not the width of a level of the tree");
    const size_t nb = (size_t)t->n_branches, nl = (size_t)t->n_leaves, n = (size_t)parents->n, nc = (size_t)out->n;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call ck(s, on_device, st);
    const unsigned long long* dbk = (const unsigned long long*)ck.in(t->branch_key, nb);
    const unsigned long long* dlk = (const unsigned long long*)ck.in(t->leaf_key, nl);
    // the table, then cell_width of expand_init / expand_gate: `width` for every parent (mode 0 reads no cell_center)
    char* w = (char*)ck.scratch(L.bytes + sizeof(float) * n);
    if (!w) return ck.error();
    float* dcw = (float*)(w + L.bytes);
    if ((rc = ck.begin(st))) return rc;
    if ((rc = octree_table_build(t, dbk, dlk, L, w, st, who))) return rc;
    if (n == 0) return ck.finish();
    Call c(s, on_device, st);
    const DevBatch P = c.batch(parents, Call::kRead), D = c.batch(out, Call::kCreate);
    const ExtendTreeOut K = extend_keys(c, keys, nc);
    if ((rc = c.begin(st))) return rc;
    const float root[4] = {t->root_center[0], t->root_center[1], t->root_center[2], t->root_width};
    const unsigned long long* tk = (const unsigned long long*)(w + L.o_keys);
    const int32_t* tv = (const int32_t*)(w + L.o_vals);
    rc = extend_enqueue(s, o, parents, P, D, width, dcw, st,
                        [&] { launch_extend_tree_pre(root, tk, tv, (uint32_t)L.slots, (int)nc, width, D, K, st); },
                        [&] { launch_extend_tree_post(root, tk, tv, (uint32_t)L.slots, (int)nc, width, D, K, st); });
    if (rc) return rc;
    if ((rc = c.finish())) return rc;
    return ck.finish();   // (waits in both forms: the table is freed when this call returns)
}
// what the host can check of a forest: the count, then the offsets, the key arrays, the roots.  A forest without trees has nothing
// more to check: it is refused with no_tree where the caller has rows that would name a tree (null: it is fine).
static int forest_host_check(const std::string& who, const hpmvs_octree_forest* f, const char* no_tree) {
    const int T = f->n_trees;
    if (T < 0) return fail(HPMVS_ERR_ARG, who + ": negative count");
    if (T == 0) return no_tree ? fail(HPMVS_ERR_ARG, who + ": " + no_tree) : HPMVS_OK;
    if (!f->root || !f->branch_first || !f->leaf_first) return fail(HPMVS_ERR_ARG, who + ": root / branch_first / leaf_first missing");
    int32_t bad = octree::forest_offsets_bad(T, f->branch_first);
    if (bad < 0) bad = octree::forest_offsets_bad(T, f->leaf_first);
    if (bad >= 0) return fail(HPMVS_ERR_ARG, who + ": tree " + std::to_string(bad) + ": the key offsets must start at 0 and never decrease");
    const size_t nb = (size_t)f->branch_first[T], nl = (size_t)f->leaf_first[T];
    if (nb + nl > ((size_t)1 << 29)) return fail(HPMVS_ERR_ARG, who + ": the forest's keys do not fit one table buffer");
    if ((nb > 0 && !f->branch_key) || (nl > 0 && !f->leaf_key)) return fail(HPMVS_ERR_ARG, who + ": key arrays missing");
    for (int k = 0; k < T; k++) {
        const float* r = f->root + 4 * (size_t)k;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]))
            return fail(HPMVS_ERR_ARG, who + ": tree " + std::to_string(k) + ": root centre not finite");
        if (!(r[3] > 0.0f) || !std::isfinite(r[3])) return fail(HPMVS_ERR_ARG, who + ": tree " + std::to_string(k) + ": root width must be finite and > 0");
    }
    return HPMVS_OK;
}
// the refusal a finding of the forest's tables (octree::forest_finding) stands for
static int forest_table_fail(const std::string& who, uint32_t finding) {
    const std::string tree = who + ": tree " + std::to_string(octree::finding_tree(finding));
    const int b = octree::finding_bad(finding);
    if (b & octree::kBadKey) return fail(HPMVS_ERR_ARG, tree + ": a word is no path key of a cell below the root (a leaf deeper than 21 levels, a branch deeper than 20)");
    if (b & octree::kBadTwice) return fail(HPMVS_ERR_ARG, tree + ": a key occurs twice (within the branch or leaf keys, or in both)");
    return fail(HPMVS_ERR_ARG, tree + ": a key's parent prefix is neither a branch nor the root");
}
// The forest's block (octree::ForestBlock) in scratch of the Call that carries the forest's arrays; f has passed
// forest_host_check.  Before begin(): the constructor declares the two key arrays, which lead the call's copies, and take() --
// behind the caller's own arrays -- the block with `tail` bytes of the caller's behind it, and fills the header's host image (hdr;
// the extra bytes are the caller's to set).  After begin(): build() uploads the header, zeroes the keys and enqueues the tables'
// build; verdict(), behind whatever kernel of the caller's folds into the same words, is the call's ONE read-back of them and the
// refusal of bad tables.  The other words are the caller's to read.
struct ForestTables {
    Call& c;
    const hpmvs_octree_forest* f;
    const octree::ForestBlock B;
    const size_t nb, nl;   // all branch / leaf keys of the forest
    const unsigned long long *dbk, *dlk;
    char* w = nullptr;
    std::vector<char> hdr;

    ForestTables(Call& c_, const hpmvs_octree_forest* f_, size_t extra_bytes)
        : c(c_), f(f_), B(octree::forest_block(f->n_trees, f->branch_first, f->leaf_first, extra_bytes)),
          nb(f->n_trees ? (size_t)f->branch_first[f->n_trees] : 0), nl(f->n_trees ? (size_t)f->leaf_first[f->n_trees] : 0),
          dbk((const unsigned long long*)c.in(f->branch_key, nb)), dlk((const unsigned long long*)c.in(f->leaf_key, nl)) {}
    bool take(size_t tail) {
        if (!(w = (char*)c.scratch(B.end + tail))) return false;
        hdr.resize(B.o_keys);
        octree::forest_block_fill(B, f->n_trees, f->root, f->branch_first, f->leaf_first, (uintptr_t)w, hdr.data());
        return true;
    }
    uint32_t* words() const { return (uint32_t*)(w + B.o_verdict); }
    const octree::Tree* trees() const { return (const octree::Tree*)(w + B.o_trees); }
    const int32_t* leaf_first() const { return (const int32_t*)(w + B.o_lf); }
    int upload(hipStream_t st) const {
        HIPCHK(hipMemcpyAsync(w, hdr.data(), B.o_keys, hipMemcpyHostToDevice, st));   // (pageable: consumed before it returns)
        HIPCHK(hipMemsetAsync(w + B.o_keys, 0, 8 * B.slots, st));
        return HPMVS_OK;
    }
    int launch(hipStream_t st) const {
        launch_forest_build(f->n_trees, (const int32_t*)(w + B.o_bf), leaf_first(), dbk, dlk, (int)(nb + nl), trees(), words(), st);
        HIPCHK(hipGetLastError());
        return HPMVS_OK;
    }
    int build(hipStream_t st) const { const int rc = upload(st); return rc ? rc : launch(st); }   // (in two steps where the caller has fills between them)
    int verdict(const std::string& who, hipStream_t st, uint32_t (&h)[kForestWords]) const {
        HIPCHK(hipMemcpyAsync(h, words(), sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return h[kForestTable] != octree::kForestGood ? forest_table_fail(who, h[kForestTable]) : HPMVS_OK;
    }
};
// The same level for ALL subtrees of a partition (kernel_extend_forest.hip): one table buffer in which every tree
// owns a slot range, one device array of {root, table}, and ONE expand_init / refinement / expand_gate for the candidates of all
// trees.  What the host knows (offsets, roots, which trees have the level) travels in one header block behind the verdict words;
// the keys' verdict and parent_tree's come back in ONE read-back, before a batch array is declared.
int hpmvs_extend_forest_batch(const hpmvs_scene* s, const hpmvs_options* o, const hpmvs_octree_forest* f, const hpmvs_patch_batch* parents,
                              const int32_t* parent_tree, float width, hpmvs_patch_batch* out, const hpmvs_extend_tree_keys* keys,
                              int on_device, void* stream) {
    const std::string who = "extend_forest_batch";
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, who + ": no HIP device visible");
    int rc = check_batch(s, o, parents);
    if (rc) return rc;
    if ((rc = check_batch_shape(s, o, out))) return rc;
    if (!f) return fail(HPMVS_ERR_ARG, who + ": null forest");
    if ((rc = extend_out_check(who, parents, out))) return rc;
    if (parents->n > 0 && !parent_tree) return fail(HPMVS_ERR_ARG, who + ": parent_tree missing");
    if (!std::isfinite(width)) return fail(HPMVS_ERR_ARG, who + ": width is not finite");
    if ((rc = forest_host_check(who, f, parents->n > 0 ? "parent_tree[0] is outside [0, n_trees): the forest has no tree" : nullptr))) return rc;
    const int T = f->n_trees;
    if (T == 0) return HPMVS_OK;
    const size_t n = (size_t)parents->n, nc = (size_t)out->n;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call ck(s, on_device, st);
    // the block's extra header bytes are has_level, one per tree; behind the block cell_width of expand_init / expand_gate
    ForestTables F(ck, f, (size_t)T);
    const int32_t* dpt = ck.in(parent_tree, n);
    if (!F.take(sizeof(float) * n)) return ck.error();
    for (int k = 0; k < T; k++) F.hdr[F.B.o_extra + k] = octree::level_depth(f->root[4 * (size_t)k + 3], width) >= 0 ? 1 : 0;
    const octree::Tree* dtrees = F.trees();
    float* dcw = (float*)(F.w + F.B.end);
    if ((rc = ck.begin(st))) return rc;
    if ((rc = F.build(st))) return rc;
    launch_forest_parents(T, (const uint8_t*)(F.w + F.B.o_extra), (int)n, dpt, F.words(), st);
    HIPCHK(hipGetLastError());
    uint32_t h[kForestWords];
    if ((rc = F.verdict(who, st, h))) return rc;
    if (h[kForestParent] != octree::kForestGood)
        return fail(HPMVS_ERR_ARG, who + ": parent_tree[" + std::to_string(h[kForestParent]) + "] is outside [0, n_trees)");
    if (h[kForestLevel] != octree::kForestGood)
        return fail(HPMVS_ERR_ARG, who + ": tree " + std::to_string(h[kForestLevel]) + ": width is not the width of a level of the tree");
    if (n == 0) return ck.finish();
    Call c(s, on_device, st);
    const DevBatch P = c.batch(parents, Call::kRead), D = c.batch(out, Call::kCreate);
    const ExtendTreeOut K = extend_keys(c, keys, nc);
    if ((rc = c.begin(st))) return rc;
    rc = extend_enqueue(s, o, parents, P, D, width, dcw, st,
                        [&] { launch_extend_forest_pre(dtrees, dpt, (int)nc, width, D, K, st); },
                        [&] { launch_extend_forest_post(dtrees, dpt, (int)nc, width, D, K, st); });
    if (rc) return rc;
    if ((rc = c.finish())) return rc;
    return ck.finish();   // (waits in both forms: the tables are freed when this call returns)
}
// One regularize / settle sweep of processCell over ALL subtrees of a partition (kernel_process_forest.hip).  Two
// Calls as above: the inputs and the call's own block first -- the forest's (ForestTables), then the leaves' owner words and the
// cells' derived arrays -- so that ONE read-back carries the forest's verdict and the cells' before an
// output is declared.  Behind it: level_support, ONE expand_init / refinement / expand_gate over all rows (the rows of a cell that
// builds nothing are skipped, as hpmvs_expand_batch skips them), the decisions, regularize against them, and the sweep's
// setDepths calls gathered on the device into ONE ordered replay.  Two more words come back mid-call, as in
// hpmvs_depth_ops_batch: the number of op rows and the number of depth keys, which size the gather and the sort.
int hpmvs_process_forest_batch(hpmvs_scene* s, const hpmvs_options* o, const hpmvs_octree_forest* f, const float* leaf_patch_center,
                               const hpmvs_patch_batch* cells, const int32_t* cell_tree, const uint64_t* cell_key, float* flatness,
                               const uint8_t* final_level, hpmvs_patch_batch* out, const hpmvs_process_forest_result* res, int on_device,
                               void* stream) {
    const std::string who = "process_forest_batch";
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, who + ": no HIP device visible");
    int rc = check_batch(s, o, cells);
    if (rc) return rc;
    if ((rc = check_batch_shape(s, o, out))) return rc;
    if (!f) return fail(HPMVS_ERR_ARG, who + ": null forest");
    if (!s->depth_pool || !s->ddepth) return fail(HPMVS_ERR_STATE, who + ": call hpmvs_scene_depth_reset first");
    if (s->depth_floats >= ((size_t)1 << 32)) return fail(HPMVS_ERR_STATE, who + ": the scene's depth maps hold 2^32 cells or more");
    const size_t n = (size_t)cells->n, M = (size_t)cells->max_images;
    if ((size_t)out->n != 4 * n) return fail(HPMVS_ERR_ARG, who + ": out->n must be 4 * cells->n");
    if (out->max_images != cells->max_images) return fail(HPMVS_ERR_ARG, who + ": max_images mismatch");
    if (5 * n * M >= ((size_t)1 << 28)) return fail(HPMVS_ERR_ARG, who + ": 5 * n * max_images must stay below 2^28 (run the sweep in pieces: the order between pieces is kept)");
    if (n > 0 && (!out->center || !out->normal || !out->scale || !out->n_images || !out->images || !out->ok))
        return fail(HPMVS_ERR_ARG, who + ": missing array");
    if (n > 0 && (!cell_tree || !cell_key || !flatness || !final_level)) return fail(HPMVS_ERR_ARG, who + ": cell_tree / cell_key / flatness / final_level missing");
    if ((rc = forest_host_check(who, f, n > 0 ? "cell 0: cell_tree is outside [0, n_trees): the forest has no tree" : nullptr))) return rc;
    const int T = f->n_trees;
    if (T == 0) return HPMVS_OK;
    const size_t nl = (size_t)f->leaf_first[T];
    if (nl > 0 && n > 0 && !leaf_patch_center) return fail(HPMVS_ERR_ARG, who + ": leaf_patch_center missing");
    // behind the forest's block: the leaves' owner words and the cells' derived arrays
    const size_t o_own = 0, o_gl = reg_align(o_own + 4 * nl), o_cc = reg_align(o_gl + 4 * n), o_cw = reg_align(o_cc + 12 * n),
                 o_skip = reg_align(o_cw + 4 * n), o_cnt = reg_align(o_skip + 4 * n), o_first = reg_align(o_cnt + 4 * (n + 1)),
                 tail = reg_align(o_first + 4 * (n + 1));
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call ck(s, on_device, st);
    ForestTables F(ck, f, 0);
    const float* dlpc = ck.in(leaf_patch_center, n > 0 ? 3 * nl : 0);
    const DevBatch P = ck.batch(cells, Call::kRead);
    ProcessCells C;
    memset(&C, 0, sizeof(C));
    C.n = (int32_t)n; C.max_images = (int32_t)M;
    C.cell_tree = ck.in(cell_tree, n);
    C.cell_key = (const unsigned long long*)ck.in(cell_key, n);
    float* dfl = ck.arr(flatness, n, Call::kCopyIn | Call::kCopyBack);
    C.flatness = dfl; C.n_images = P.n_images; C.images = P.images;
    const uint8_t* dfinal = ck.in(final_level, n);
    if (!F.take(tail)) return ck.error();
    size_t scan_bytes = 0;
    if (process_scan(nullptr, &scan_bytes, nullptr, nullptr, (int)n + 1, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM size query failed");
    void* scan_temp = ck.scratch(scan_bytes ? scan_bytes : 1);
    if (!scan_temp) return ck.error();
    const octree::Tree* dtrees = F.trees();
    const int32_t* dlf = F.leaf_first();
    char* w = F.w + F.B.end;
    C.owner = (int32_t*)(w + o_own); C.gleaf = (int32_t*)(w + o_gl);
    C.cell_center = (float*)(w + o_cc); C.cell_width = (float*)(w + o_cw);
    uint8_t* dskip = (uint8_t*)(w + o_skip);
    int32_t* op_count = (int32_t*)(w + o_cnt);
    int32_t* op_first = (int32_t*)(w + o_first);
    if ((rc = ck.begin(st))) return rc;
    if ((rc = F.upload(st))) return rc;
    if (nl) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)C.owner, octree::kNoOwner, nl, st));
    if ((rc = F.launch(st))) return rc;
    launch_process_cells(T, dtrees, dlf, s->n_views, C, F.words(), st);
    HIPCHK(hipGetLastError());
    uint32_t h[kForestWords];
    if ((rc = F.verdict(who, st, h))) return rc;
    if (h[kForestParent] != octree::kForestGood) {
        const std::string cell = who + ": cell " + std::to_string(h[kForestParent] >> 3);
        switch (h[kForestParent] & 7u) {
            case octree::kCellTree: return fail(HPMVS_ERR_ARG, cell + ": cell_tree is outside [0, n_trees)");
            case octree::kCellLeaf: return fail(HPMVS_ERR_ARG, cell + ": cell_key is no nonempty leaf of its tree");
            case octree::kCellTwice: return fail(HPMVS_ERR_ARG, cell + ": its leaf belongs to an earlier cell already (a leaf changes at most once per sweep)");
            case octree::kCellDeep: return fail(HPMVS_ERR_ARG, cell + ": a leaf at depth 21 cannot be branched");
            default: return fail(HPMVS_ERR_ARG, cell + ": a regularized cell's reference image is not a view of the scene");
        }
    }
    if (n == 0) return ck.finish();
    Call c(s, on_device, st);
    const DevBatch D = c.batch(out, Call::kCreate);
    static const hpmvs_process_forest_result none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const hpmvs_process_forest_result& R = res ? *res : none;
    // what the sweep itself needs lives in scratch where the caller does not ask for it
    auto result = [&c](auto* given, size_t count) {
        auto* p = c.arr(given, count, Call::kCopyBack);
        return p ? p : (decltype(p))c.scratch(sizeof(*p) * count);
    };
    int32_t* dsup = result(R.support, n);
    C.removed = result(R.removed, n);
    C.split = result(R.split, n);
    C.children = result(R.children, 4 * n);
    C.child_key = (unsigned long long*)result(R.child_key, 4 * n);
    int32_t* dnn = c.arr(R.n_neighbours, n, Call::kCopyBack);
    unsigned long long* dnk = (unsigned long long*)c.arr(R.neighbour_key, 24 * n, Call::kCopyBack);
    if (c.error()) return c.error();
    if ((rc = c.begin(st))) return rc;
    const DevOptions d = make_dev_options(o);
    const DevScene sc = dev_scene(s);
    launch_level_support(sc, P, o->MINLEVEL, dsup, st);
    HIPCHK(hipGetLastError());
    launch_process_skip(C, dsup, dskip, st);
    HIPCHK(hipGetLastError());
    {
        std::lock_guard<std::recursive_mutex> lk(s->mu);
        launch_expand_init(sc, HPMVS_EXPAND_BRANCH, (int)n, P, C.cell_center, C.cell_width, dskip, D, st);
        HIPCHK(hipGetLastError());
        if ((rc = enqueue_refinement(s, d, D, st))) return rc;
        launch_expand_gate(HPMVS_EXPAND_BRANCH, (int)n, P, C.cell_center, C.cell_width, D, st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(op_count + n, 0, 4, st));
    launch_process_decide(C, dsup, dskip, dfinal, D, op_count, st);
    HIPCHK(hipGetLastError());
    launch_regularize_forest(sc, dtrees, dlf, dlpc, C, P, D, dfl, dnn, dnk, st);
    HIPCHK(hipGetLastError());
    if (process_scan(scan_temp, &scan_bytes, op_count, op_first, (int)n + 1, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM scan failed");
    int32_t n_ops = 0;   // the op batch's size depends on it: read back mid-call
    HIPCHK(hipMemcpyAsync(&n_ops, op_first + n, sizeof(n_ops), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_ops > 0) {
        const size_t m = (size_t)n_ops, cap = m * M;
        DevBatch ops;
        memset(&ops, 0, sizeof(ops));
        ops.n = n_ops; ops.max_images = (int32_t)M;
        char* ob = (char*)c.scratch(reg_align(16 * m) * 2 + reg_align(4 * m) * 2 + reg_align(4 * cap) + reg_align(m));
        unsigned long long* keys = (unsigned long long*)c.scratch(cap * sizeof(unsigned long long));
        unsigned long long* sorted = (unsigned long long*)c.scratch(cap * sizeof(unsigned long long));
        unsigned int* counter = (unsigned int*)c.scratch(sizeof(unsigned int));
        if (c.error()) return c.error();
        ops.center = (float*)ob; ops.normal = (float*)(ob + reg_align(16 * m)); ops.scale = (float*)((char*)ops.normal + reg_align(16 * m));
        ops.n_images = (int32_t*)((char*)ops.scale + reg_align(4 * m)); ops.images = (int32_t*)((char*)ops.n_images + reg_align(4 * m));
        uint8_t* dsub = (uint8_t*)((char*)ops.images + reg_align(4 * cap));
        launch_process_gather(C, op_first, P, D, ops, dsub, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned int), st));
        launch_depth_ops_keys(sc, s->ddepth, s->depth_pool, ops, keys, counter, st);
        HIPCHK(hipGetLastError());
        unsigned int count = 0;  // the sort's size depends on it
        HIPCHK(hipMemcpyAsync(&count, counter, sizeof(count), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (count > 0) {
            size_t temp_bytes = 0;
            if (depth_ops_sort(nullptr, &temp_bytes, keys, sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM size query failed");
            void* temp = c.scratch(temp_bytes ? temp_bytes : 1);
            if (!temp) return c.error();
            if (depth_ops_sort(temp, &temp_bytes, keys, sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM sort failed");
            launch_depth_ops_apply(sc, s->ddepth, s->depth_pool, ops, dsub, sorted, count, st);
            HIPCHK(hipGetLastError());
        }
    }
    if ((rc = c.finish())) return rc;
    return ck.finish();   // (waits in both forms: the tables are freed when this call returns; flatness travels back here)
}
// A round's border queue over ALL subtrees (kernel_border_forest.hip): distributeBorderCell, every tree's
// processBorderCellQueue and the accepted patches' setDepths(p, false) as ONE call.  One Call: no array is filled by begin() (the
// kernels write every entry of every output), so declaring the outputs ahead of the verdict writes nothing; the forest's verdict
// comes back in ONE read-back before the first kernel that touches an output or a map is enqueued.  The scratch is the call's own:
// the forest's block (ForestTables), then 56 bytes per patch and rocPRIM's temporary storage.
int hpmvs_border_forest_batch(hpmvs_scene* s, const hpmvs_octree_forest* f, const hpmvs_patch_batch* border, int set_depths,
                              const hpmvs_border_forest_result* res, int on_device, void* stream) {
    const std::string who = "border_forest_batch";
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, who + ": no HIP device visible");
    if (!s || !f || !border) return fail(HPMVS_ERR_ARG, who + ": null scene / forest / batch");
    if (!s->committed) return fail(HPMVS_ERR_STATE, who + ": scene not committed");
    if (border->n < 0 || border->max_images < 1 || border->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, who + ": bad n/max_images");
    if (border->n > 0 && (!border->center || !border->scale)) return fail(HPMVS_ERR_ARG, who + ": batch input arrays missing (center / scale)");
    if (border->n > 0 && set_depths && (!border->normal || !border->n_images || !border->images))
        return fail(HPMVS_ERR_ARG, who + ": batch input arrays missing (set_depths reads normal / n_images / images)");
    int rc;
    if ((rc = forest_host_check(who, f, nullptr))) return rc;   // (no tree: every patch is routed nowhere)
    if (set_depths && (!s->depth_pool || !s->ddepth)) return fail(HPMVS_ERR_STATE, who + ": call hpmvs_scene_depth_reset first");
    const int T = f->n_trees;
    const size_t n = (size_t)border->n, M = (size_t)border->max_images;
    if (T == 0 && n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    ForestTables F(c, f, 0);
    DevBatch D;
    memset(&D, 0, sizeof(D));
    D.n = border->n; D.max_images = border->max_images;
    D.center = c.in(border->center, 4 * n);
    D.scale = c.in(border->scale, n);
    if (set_depths) {
        D.n_images = c.in(border->n_images, n);
        D.images = c.in(border->images, n * M);
    }
    static const hpmvs_border_forest_result none = {nullptr, nullptr, nullptr, nullptr};
    const hpmvs_border_forest_result& R = res ? *res : none;
    BorderForestOut out;   // (the static and the replay kernel between them write every entry: no zero fill)
    out.tree = c.arr(R.tree, n, Call::kCopyBack);
    out.accepted = c.arr(R.accepted, n, Call::kCopyBack);
    out.leaf_key = (unsigned long long*)c.arr(R.leaf_key, n, Call::kCopyBack);
    out.blocker = c.arr(R.blocker, n, Call::kCopyBack);
    if (c.error()) return c.error();
    if (set_depths && n > 0 && !out.accepted) {   // the mask of set_depths_kernel, in scratch where the caller does not ask for it
        out.accepted = (uint8_t*)c.scratch(n);
        if (!out.accepted) return c.error();
    }
    if (!F.take(0)) return c.error();
    BorderForestScratch S;
    memset(&S, 0, sizeof(S));
    if (n > 0) {
        S.temp_bytes = border_forest_temp_bytes((int)n, T);
        if (S.temp_bytes == (size_t)-1) return fail(HPMVS_ERR_HIP, who + ": rocPRIM size query failed");
        // one block: four 8-byte arrays, six 4-byte ones, then rocPRIM's temporary storage
        const size_t o_temp = reg_align(56 * n);
        char* blk = (char*)c.scratch(o_temp + S.temp_bytes);
        if (!blk) return c.error();
        S.path = (unsigned long long*)blk; S.key_a = S.path + n; S.key_b = S.key_a + n; S.acc_key = S.key_b + n;
        S.val_a = (uint32_t*)(S.acc_key + n); S.val_b = S.val_a + n; S.tree_a = S.val_b + n; S.tree_b = S.tree_a + n; S.tree_c = S.tree_b + n;
        S.acc_owner = (int32_t*)(S.tree_c + n);
        S.temp = blk + o_temp;
    }
    if ((rc = c.begin(st))) return rc;
    if (T) {   // (without a tree the block is never read: nothing to upload or build)
        uint32_t h[kForestWords];
        if ((rc = F.build(st)) || (rc = F.verdict(who, st, h))) return rc;
    }
    if (n > 0) {
        if (launch_border_forest(T, F.trees(), (int)n, D.center, D.scale, S, out, st)) return fail(HPMVS_ERR_HIP, who + ": rocPRIM sort failed");
        HIPCHK(hipGetLastError());
        if (set_depths) {
            D.ok = out.accepted;
            launch_set_depths(dev_scene(s), s->ddepth, D, st);
            HIPCHK(hipGetLastError());
        }
    }
    return c.finish();   // (waits in both forms: the tables and the scratch are freed when this call returns)
}
// CellProcessor::processBorderCellQueue's insertion loop (CellProcessor.cpp:500-531): addConditional(points[i], add_width[i]) for
// i = 0 .. n - 1 IN THAT ORDER against the tree t, which stays the caller's (kernel_octree_insert.hip: static kernel, stable sort by
// static leaf, one wavefront per leaf's run).  The scratch is the call's own, sized by n alone.
int hpmvs_octree_insert_batch(const hpmvs_scene* s, const hpmvs_octree_index* t, int n, const float* points, const float* add_width,
                              uint8_t* accepted, uint64_t* leaf_key, int32_t* blocker, int on_device, void* stream) {
    const char* who = "octree_insert_batch";
    OctreeLayout L;
    int rc = octree_index_check(s, t, n, points, who, &L);
    if (rc) return rc;
    if (n > 0 && (!add_width || !accepted || !leaf_key)) return fail(HPMVS_ERR_ARG, "octree_insert_batch: add_width / accepted / leaf_key missing");
    const size_t nb = (size_t)t->n_branches, nl = (size_t)t->n_leaves, np = (size_t)n;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const unsigned long long* dbk = (const unsigned long long*)c.in(t->branch_key, nb);
    const unsigned long long* dlk = (const unsigned long long*)c.in(t->leaf_key, nl);
    const float* dpts = c.in(points, 3 * np);
    const float* daw = c.in(add_width, np);
    OctreeInsertOut out;   // (the static and the replay kernel between them write every entry: no zero fill)
    out.accepted = c.arr(accepted, np, Call::kCopyBack);
    out.leaf_key = (unsigned long long*)c.arr(leaf_key, np, Call::kCopyBack);
    out.blocker = c.arr(blocker, np, Call::kCopyBack);
    OctreeInsertScratch S;
    memset(&S, 0, sizeof(S));
    if (n > 0) {
        S.temp_bytes = octree_insert_temp_bytes(n);
        if (S.temp_bytes == (size_t)-1) return fail(HPMVS_ERR_HIP, "octree_insert_batch: rocPRIM size query failed");
        // one block: four 8-byte arrays, three 4-byte ones, then rocPRIM's temporary storage
        const size_t o_temp = reg_align(44 * np);
        char* blk = (char*)c.scratch(o_temp + S.temp_bytes);
        if (!blk) return c.error();
        S.path = (unsigned long long*)blk; S.key_a = S.path + np; S.key_b = S.key_a + np; S.acc_key = S.key_b + np;
        S.val_a = (uint32_t*)(S.acc_key + np); S.val_b = S.val_a + np; S.acc_owner = (int32_t*)(S.val_b + np);
        S.temp = blk + o_temp;
    }
    if ((rc = c.begin(st))) return rc;
    WorkspaceTable tt(s, t, dbk, dlk, L, st, who);
    if (tt.rc) return tt.rc;
    if (launch_octree_insert(tt.root, tt.keys, tt.vals, tt.slots, n, dpts, daw, S, out, st))
        return fail(HPMVS_ERR_HIP, "octree_insert_batch: rocPRIM sort failed");
    HIPCHK(hipGetLastError());
    return c.finish();   // (waits in both forms: the scratch is freed when this call returns)
}
// getSubTrees(tree, list, min_trees) and cellHistogram (src/main.cpp:50-96, doctree.h:493-523) for the tree t
// (kernel_octree_partition.hip: leaf kernel, sort by aligned key, the loop on one wavefront, assignment).  The scratch is the
// call's own; the one read-back after the table's verdict is the device record.
static_assert(sizeof(hpmvs_octree_partition_info) == 4 * kPartitionInts && HPMVS_MAX_SUBTREES == octree::kMaxSubtrees &&
              HPMVS_MAX_TREE_DEPTH == octree::kMaxDepth, "hpmvs_octree_partition_info is the device record");
int hpmvs_octree_partition(const hpmvs_scene* s, const hpmvs_octree_index* t, int min_trees, int min_split_leaves,
                           hpmvs_octree_partition_info* info, uint64_t* root_key, float* root_cell, int32_t* tree_first,
                           int32_t* tree_leaves, int32_t* leaf_order, int32_t* leaf_tree, uint64_t* leaf_sub_key, int32_t* branch_tree,
                           uint64_t* branch_sub_key, int on_device, void* stream) {
    const char* who = "octree_partition";
    OctreeLayout L;
    int rc = octree_index_check(s, t, 0, nullptr, who, &L);
    if (rc) return rc;
    if (!info) return fail(HPMVS_ERR_ARG, "octree_partition: info missing");
    if (min_trees > HPMVS_MAX_SUBTREES) return fail(HPMVS_ERR_ARG, "octree_partition: min_trees exceeds HPMVS_MAX_SUBTREES");
    if (min_split_leaves < 1) return fail(HPMVS_ERR_ARG, "octree_partition: min_split_leaves must be >= 1");
    const size_t nb = (size_t)t->n_branches, nl = (size_t)t->n_leaves;
    const int cap = min_trees + 6 > 8 ? min_trees + 6 : 8;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const unsigned long long* dbk = (const unsigned long long*)c.in(t->branch_key, nb);
    const unsigned long long* dlk = (const unsigned long long*)c.in(t->leaf_key, nl);
    OctreePartitionRoots roots;   // (the kernels write every entry of every output they are given: no zero fill)
    roots.root_key = (unsigned long long*)c.arr(root_key, (size_t)cap, Call::kCopyBack);
    roots.root_cell = c.arr(root_cell, 4 * (size_t)cap, Call::kCopyBack);
    roots.tree_first = c.arr(tree_first, (size_t)cap, Call::kCopyBack);
    roots.tree_leaves = c.arr(tree_leaves, (size_t)cap, Call::kCopyBack);
    int32_t* dorder = c.arr(leaf_order, nl, Call::kCopyBack);
    OctreePartitionKeys out;
    out.leaf_tree = c.arr(leaf_tree, nl, Call::kCopyBack);
    out.leaf_sub_key = (unsigned long long*)c.arr(leaf_sub_key, nl, Call::kCopyBack);
    out.branch_tree = c.arr(branch_tree, nb, Call::kCopyBack);
    out.branch_sub_key = (unsigned long long*)c.arr(branch_sub_key, nb, Call::kCopyBack);
    OctreePartitionScratch S;
    memset(&S, 0, sizeof(S));
    S.temp_bytes = octree_partition_temp_bytes((int)nl);
    if (S.temp_bytes == (size_t)-1) return fail(HPMVS_ERR_HIP, "octree_partition: rocPRIM size query failed");
    S.root_slots = octree::table_slots((size_t)cap);
    // one block: the record and the root table (zeroed), two 8-byte and two 4-byte arrays per leaf, then rocPRIM's temporary storage
    const size_t o_rk = reg_align(4 * kPartitionInts), o_rv = o_rk + 8 * (size_t)S.root_slots, o_ka = reg_align(o_rv + 4 * (size_t)S.root_slots);
    const size_t o_temp = reg_align(o_ka + 24 * nl);
    char* blk = (char*)c.scratch(o_temp + S.temp_bytes);
    if (!blk) return c.error();
    S.info = (int32_t*)blk;
    S.root_keys = (unsigned long long*)(blk + o_rk); S.root_vals = (int32_t*)(blk + o_rv);
    S.key_a = (unsigned long long*)(blk + o_ka); S.key_b = S.key_a + nl;
    S.val_a = (int32_t*)(S.key_b + nl); S.val_b = S.val_a + nl;
    S.temp = blk + o_temp;
    if ((rc = c.begin(st))) return rc;
    WorkspaceTable tt(s, t, dbk, dlk, L, st, who);
    if (tt.rc) return tt.rc;
    HIPCHK(hipMemsetAsync(blk, 0, o_ka, st));
    if (launch_octree_partition(tt.root, tt.keys, tt.vals, tt.slots, dbk, (int)nb, dlk, (int)nl, min_trees, min_split_leaves, cap, S, roots, dorder,
                                out, st))
        return fail(HPMVS_ERR_HIP, "octree_partition: rocPRIM sort failed");
    HIPCHK(hipGetLastError());
    int32_t h[kPartitionInts];
    HIPCHK(hipMemcpyAsync(h, S.info, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(info, h, sizeof(*info));
    return c.finish();   // (waits in both forms: the scratch is freed when this call returns)
}
// distributeBorderCell's search (CellProcessor.cpp:487-498, 533-540): the first root in list order that contains the point.  The
// roots are a host array in both forms, like an hpmvs_octree_index: they are checked here and travel in the call's scratch.
int hpmvs_octree_route_batch(const hpmvs_scene* s, int n_trees, const float* roots, int n, const float* points, int32_t* tree, int on_device,
                             void* stream) {
    if (hpmvs_device_count() <= 0) return fail(HPMVS_ERR_NODEVICE, "octree_route_batch: no HIP device visible");
    if (!s) return fail(HPMVS_ERR_ARG, "octree_route_batch: null scene");
    if (!s->committed) return fail(HPMVS_ERR_STATE, "octree_route_batch: scene not committed");
    if (n < 0 || n_trees < 0) return fail(HPMVS_ERR_ARG, "octree_route_batch: negative count");
    if ((n_trees > 0 && !roots) || (n > 0 && (!points || !tree))) return fail(HPMVS_ERR_ARG, "octree_route_batch: roots / points / tree missing");
    for (int k = 0; k < 4 * n_trees; k++)
        if (!std::isfinite(roots[k]) || (k % 4 == 3 && !(roots[k] > 0.0f)))
            return fail(HPMVS_ERR_ARG, "octree_route_batch: a root is not finite or has no positive width");
    if (n == 0) return HPMVS_OK;
    int rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const float* dpts = c.in(points, 3 * (size_t)n);
    int32_t* dtree = c.arr(tree, (size_t)n, Call::kCopyBack);   // (every entry is written)
    float* droots = n_trees ? (float*)c.scratch(16 * (size_t)n_trees) : nullptr;
    if (n_trees && !droots) return c.error();
    if ((rc = c.begin(st))) return rc;
    if (n_trees) HIPCHK(hipMemcpyAsync(droots, roots, 16 * (size_t)n_trees, hipMemcpyHostToDevice, st));   // (pageable: consumed before it returns)
    launch_octree_route(n_trees, droots, n, dpts, dtree, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}
int hpmvs_depth_gates_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, float margin, int abs_int,
                            int32_t* n_visible, int32_t* n_blocking, int32_t* n_free, int on_device, void* stream) {
    int rc = check_depth_batch(s, b, "depth_gates_batch");
    if (rc) return rc;
    if (!n_visible && !n_blocking && !n_free) return fail(HPMVS_ERR_ARG, "depth_gates_batch: no output array");
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const size_t n = (size_t)b->n;
    const DevBatch D = c.batch(b, Call::kRead);
    int32_t *dv = c.out(n_visible, n), *db = c.out(n_blocking, n), *df = c.out(n_free, n);
    if ((rc = c.begin())) return rc;
    launch_depth_gates(dev_scene(s), s->ddepth, D, margin, abs_int, dv, db, df, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}

int hpmvs_depth_footprints_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, int32_t* writes, int32_t* frees,
                                 int32_t* attached, int32_t* view_block, int on_device, void* stream) {
    int rc = check_depth_batch(s, b, "depth_footprints_batch");
    if (rc) return rc;
    if (!writes && !frees && !attached && !view_block) return fail(HPMVS_ERR_ARG, "depth_footprints_batch: no output array");
    if (b->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    Call c(s, on_device, st);
    const size_t n = (size_t)b->n, M = (size_t)b->max_images, V = (size_t)s->n_views;
    const DevBatch D = c.batch(b, Call::kRead);
    int32_t *dw = c.out(writes, n * M * 4), *df = c.out(frees, n * M * 4);
    int32_t *da = c.out(attached, n * M * 3), *dv = c.out(view_block, n * V * 3);
    if ((rc = c.begin())) return rc;
    launch_depth_footprints(dev_scene(s), s->ddepth, D, dw, df, da, dv, st);
    HIPCHK(hipGetLastError());
    return c.finish();
}

// An extend level's conflict graph (kernel_conflicts.hip, conflicts.hpp).  conflicts_call is the part the two
// entry points share: the graph of device footprints F into the caller's CSR arrays.  The offsets and the totals are always
// written; the adjacency arrays only when both capacities suffice (host pointers: they are staged here, so a call that fails on
// capacity leaves the caller's arrays as they were).  n_flow / n_anti are host words in both forms.
static int conflicts_check(const std::string& who, long long n, int M, int V, int n_levels, const uint32_t* flow_off, const uint32_t* flow_adj,
                           size_t cap_flow, const uint32_t* anti_off, const uint32_t* anti_adj, size_t cap_anti, const uint32_t* n_flow,
                           const uint32_t* n_anti) {
    if (n < 0) return fail(HPMVS_ERR_ARG, who + ": negative n");
    if (M < 1 || M > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, who + ": max_images outside 1 .. HPMVS_MAX_IMAGES");
    if (V < 1 || V > conflicts::kMaxViews) return fail(HPMVS_ERR_ARG, who + ": the number of views is outside 1 .. 8191");
    if (n_levels < 1 || n_levels > HPMVS_MAX_LEVELS) return fail(HPMVS_ERR_ARG, who + ": n_levels outside 1 .. HPMVS_MAX_LEVELS");
    if (n * (long long)M >= (1ll << 28)) return fail(HPMVS_ERR_ARG, who + ": n * max_images must be below 2^28");
    if (!flow_off || !anti_off || !n_flow || !n_anti) return fail(HPMVS_ERR_ARG, who + ": flow_off / anti_off / n_flow / n_anti missing");
    if ((cap_flow && !flow_adj) || (cap_anti && !anti_adj)) return fail(HPMVS_ERR_ARG, who + ": an adjacency array is null but has a capacity");
    return HPMVS_OK;
}
static int conflicts_call(Call& c, const std::string& who, const conflicts::Footprints& F, int on_device, uint32_t* dflow_off, uint32_t* flow_adj,
                          size_t cap_flow, uint32_t* danti_off, uint32_t* anti_adj, size_t cap_anti, uint32_t* n_flow, uint32_t* n_anti,
                          hipStream_t st) {
    const unsigned long long* pairs = nullptr;
    uint32_t nf = 0, na = 0;
    const int rc = launch_conflicts(F, [&c](size_t bytes) { return c.scratch(bytes); }, dflow_off, danti_off, &pairs, &nf, &na, st);
    if (rc == kConflictsMemory) return c.error() ? c.error() : fail(HPMVS_ERR_HIP, who + ": out of device memory");
    if (rc == kConflictsTooMany)
        return fail(HPMVS_ERR_STATE, who + ": more than 2^30 conflicting (reader, writer) pairs before duplicates are dropped");
    if (rc != kConflictsOk) return fail(HPMVS_ERR_HIP, who + ": " + hipGetErrorString(hipGetLastError()));
    *n_flow = nf; *n_anti = na;
    const bool fits = nf <= cap_flow && na <= cap_anti;
    if (fits && nf + (size_t)na) {
        uint32_t *df = flow_adj, *da = anti_adj;
        if (!on_device) {
            df = nf ? (uint32_t*)c.scratch(4 * (size_t)nf) : nullptr; da = na ? (uint32_t*)c.scratch(4 * (size_t)na) : nullptr;
            if ((nf && !df) || (na && !da)) return c.error();
        }
        launch_conflicts_adjacency(pairs, nf, na, df, da, st);
        HIPCHK(hipGetLastError());
        if (!on_device) {
            HIPCHK(hipStreamSynchronize(st));
            if (nf) HIPCHK(hipMemcpy(flow_adj, df, 4 * (size_t)nf, hipMemcpyDeviceToHost));
            if (na) HIPCHK(hipMemcpy(anti_adj, da, 4 * (size_t)na, hipMemcpyDeviceToHost));
        }
    }
    const int done = c.finish();   // (the offsets travel back here; waits in both forms: the scratch is freed on return)
    if (done) return done;
    if (!fits) return fail(HPMVS_ERR_ARG, who + ": capacity: the graph has " + std::to_string(nf) + " flow and " + std::to_string(na) +
                                              " anti entries (n_flow / n_anti are set; allocate and call again)");
    return HPMVS_OK;
}
// n == 0: the empty graph
static int conflicts_empty(int on_device, uint32_t* flow_off, uint32_t* anti_off, uint32_t* n_flow, uint32_t* n_anti, hipStream_t st) {
    if (on_device) {
        HIPCHK(hipMemsetAsync(flow_off, 0, 4, st));
        HIPCHK(hipMemsetAsync(anti_off, 0, 4, st));
    } else { flow_off[0] = 0; anti_off[0] = 0; }
    *n_flow = 0; *n_anti = 0;
    return HPMVS_OK;
}

int hpmvs_conflicts_from_footprints(int device, int n, int max_images, int n_views, int n_levels, const int32_t* n_images, const int32_t* writes,
                                    const int32_t* frees, const int32_t* attached, const int32_t* view_block, const uint8_t* is_event,
                                    uint32_t* flow_off, uint32_t* flow_adj, size_t cap_flow, uint32_t* anti_off, uint32_t* anti_adj,
                                    size_t cap_anti, uint32_t* n_flow, uint32_t* n_anti, int on_device, void* stream) {
    const std::string who = "conflicts_from_footprints";
    int rc = conflicts_check(who, n, max_images, n_views, n_levels, flow_off, flow_adj, cap_flow, anti_off, anti_adj, cap_anti, n_flow, n_anti);
    if (rc) return rc;
    if (n > 0 && (!n_images || !writes || !frees || !attached || !view_block)) return fail(HPMVS_ERR_ARG, who + ": a footprint array is null");
    const int count = hpmvs_device_count();
    if (count <= 0) return fail(HPMVS_ERR_NODEVICE, who + ": no HIP device visible");
    if (device < 0 || device >= count) return fail(HPMVS_ERR_ARG, who + ": no such device");
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return conflicts_empty(on_device, flow_off, anti_off, n_flow, n_anti, st);
    Call c(nullptr, on_device, st);
    const size_t N = (size_t)n, M = (size_t)max_images, V = (size_t)n_views;
    conflicts::Footprints F;
    F.n = n; F.M = max_images; F.V = n_views; F.n_levels = n_levels;
    F.n_images = c.in(n_images, N);
    F.wr = c.in(writes, N * M * 4); F.fr = c.in(frees, N * M * 4); F.at = c.in(attached, N * M * 3); F.vb = c.in(view_block, N * V * 3);
    F.is_event = c.in(is_event, N);
    uint32_t* dfo = c.arr(flow_off, N + 1, Call::kCopyBack);   // (every offset is written)
    uint32_t* dao = c.arr(anti_off, N + 1, Call::kCopyBack);
    if ((rc = c.begin())) return rc;
    return conflicts_call(c, who, F, on_device, dfo, flow_adj, cap_flow, dao, anti_adj, cap_anti, n_flow, n_anti, st);
}

int hpmvs_level_conflicts_batch(const hpmvs_scene* s, const hpmvs_patch_batch* b, const uint8_t* is_event, uint32_t* flow_off, uint32_t* flow_adj,
                                size_t cap_flow, uint32_t* anti_off, uint32_t* anti_adj, size_t cap_anti, uint32_t* n_flow, uint32_t* n_anti,
                                int on_device, void* stream) {
    const std::string who = "level_conflicts_batch";
    int rc = check_depth_batch(s, b, who.c_str());
    if (rc) return rc;
    // the levels a read can be on: the deepest pyramid of the scene's cameras (what getFullDepth walks)
    int n_levels = 1;
    for (int v = 0; v < s->n_views; v++) n_levels = std::max(n_levels, (int)s->hviews[v].n_levels);
    if ((rc = conflicts_check(who, b->n, b->max_images, s->n_views, n_levels, flow_off, flow_adj, cap_flow, anti_off, anti_adj, cap_anti, n_flow, n_anti)))
        return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (b->n == 0) return conflicts_empty(on_device, flow_off, anti_off, n_flow, n_anti, st);
    Call c(s, on_device, st);
    const size_t N = (size_t)b->n, M = (size_t)b->max_images, V = (size_t)s->n_views;
    const DevBatch D = c.batch(b, Call::kRead);
    const uint8_t* dev = c.in(is_event, N);
    uint32_t* dfo = c.arr(flow_off, N + 1, Call::kCopyBack);
    uint32_t* dao = c.arr(anti_off, N + 1, Call::kCopyBack);
    // the footprints never leave the device: one block of scratch, cut into the four arrays
    int32_t* fp = (int32_t*)c.scratch(4 * N * (11 * M + 3 * V));
    if (!fp) return c.error();
    if ((rc = c.begin())) return rc;
    conflicts::Footprints F;
    F.n = b->n; F.M = b->max_images; F.V = s->n_views; F.n_levels = n_levels;
    F.n_images = D.n_images; F.is_event = dev;
    int32_t *wr = fp, *fr = wr + N * M * 4, *at = fr + N * M * 4, *vb = at + N * M * 3;
    F.wr = wr; F.fr = fr; F.at = at; F.vb = vb;
    launch_depth_footprints(dev_scene(s), s->ddepth, D, wr, fr, at, vb, st);
    HIPCHK(hipGetLastError());
    return conflicts_call(c, who, F, on_device, dfo, flow_adj, cap_flow, dao, anti_adj, cap_anti, n_flow, n_anti, st);
}

// The wave walk of one extend level, entirely on the device (kernel_level_walk.hip, level_walk.hpp): the graph by
// the device code of hpmvs_level_conflicts_batch, the key records, then per wave the gates over the pending refined candidates,
// resolve rounds, and ONE ordered depth update.  The host reads a count per wave and per round and decides nothing but when to stop.
static constexpr int kWalkFewDecided = 8;      // a round that decided fewer items, with at most kWalkFinishBudget left, is followed by
static constexpr int kWalkFinishBudget = 128;  // an in-order pass of one wavefront that decides them all: the end of a chain
int hpmvs_level_walk_batch(hpmvs_scene* s, const hpmvs_options* o, const hpmvs_patch_batch* items, const uint8_t* flags, const int32_t* set,
                           const uint64_t* pre_key, const uint64_t* post_key, float margin, int abs_int, int32_t* stage, int32_t* counts,
                           uint8_t* accepted, int32_t* wave, int32_t* n_waves, int on_device, void* stream) {
    const std::string who = "level_walk_batch";
    if (!s || !o || !items || !n_waves) return fail(HPMVS_ERR_ARG, who + ": null scene / options / batch / n_waves");
    if (items->n < 0 || items->max_images < 1 || items->max_images > HPMVS_MAX_IMAGES) return fail(HPMVS_ERR_ARG, who + ": bad n/max_images");
    if (items->n > 0 && (!items->center || !items->normal || !items->scale || !items->n_images || !items->images))
        return fail(HPMVS_ERR_ARG, who + ": batch input arrays missing");
    if (items->n > 0 && (!flags || !pre_key || !post_key || !stage || !counts || !accepted || !wave))
        return fail(HPMVS_ERR_ARG, who + ": flags / pre_key / post_key / stage / counts / accepted / wave missing");
    if (o->MIN_IMAGES_PER_PATCH < 1) return fail(HPMVS_ERR_ARG, who + ": MIN_IMAGES_PER_PATCH must be >= 1");
    int n_levels = 1;
    for (int v = 0; v < s->n_views; v++) n_levels = std::max(n_levels, (int)s->hviews[v].n_levels);
    {   // whatever hpmvs_level_conflicts_batch refuses (the graph is over at most n nodes)
        uint32_t off = 0, total = 0;
        const int rc = conflicts_check(who, items->n, items->max_images, s->n_views, n_levels, &off, nullptr, 0, &off, nullptr, 0, &total, &total);
        if (rc) return rc;
    }
    if (!s->committed || !s->depth_pool || !s->ddepth) return fail(HPMVS_ERR_STATE, who + ": call hpmvs_scene_depth_reset first");
    if (s->depth_floats >= ((size_t)1 << 32)) return fail(HPMVS_ERR_STATE, who + ": the scene's depth maps hold 2^32 cells or more");
    *n_waves = 0;
    for (auto& w : s->last_walk) w = 0;
    if (items->n == 0) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int rc;
    Call c(s, on_device, st);
    const int n = items->n, M = items->max_images, V = s->n_views;
    const size_t N = (size_t)n;
    const DevBatch D = c.batch(items, Call::kRead);
    const uint8_t* dflags = c.in(flags, N);
    const int32_t* dset = c.in(set, N);
    const unsigned long long *dpre = c.in((const unsigned long long*)pre_key, N), *dpost = c.in((const unsigned long long*)post_key, N);
    // outputs: nothing of the caller's is written before walk_init_kernel, so no zero fill and no copy back on a refusal
    int32_t* dstage = c.arr(stage, N, Call::kCopyIn | Call::kCopyBack);
    int32_t* dcounts = c.arr(counts, 3 * N, Call::kCopyBack);
    uint8_t* daccepted = c.arr(accepted, N, Call::kCopyBack);
    int32_t* dwave = c.arr(wave, N, Call::kCopyBack);
    // the call's own arrays, one block: sizes known from n (a node batch has at most n rows)
    size_t need = 0;
    auto room = [&need](size_t bytes) { const size_t at = need; need += reg_align(bytes); return at; };
    const size_t a_ctl = room(64), a_state = room(N), a_ok = room(N), a_sub = room(N), a_nev = room(N), a_mark = room(4 * N), a_scan = room(4 * N),
                 a_node = room(4 * N), a_item = room(4 * N), a_slot = room(4 * N), a_rows = room(4 * N), a_gv = room(4 * N), a_gb = room(4 * N),
                 a_gf = room(4 * N), a_fpre = room(4 * N), a_fpost = room(4 * N), a_foff = room(4 * (N + 1)), a_aoff = room(4 * (N + 1)),
                 a_k0 = room(16 * N), a_k1 = room(16 * N), a_key = room(16 * N), a_v0 = room(8 * N), a_v1 = room(8 * N), a_val = room(8 * N),
                 a_s0 = room(8 * N), a_set = room(8 * N), a_p0 = room(8 * N), a_perm = room(8 * N), a_bc = room(16 * N), a_bn = room(16 * N),
                 a_bs = room(4 * N), a_bi = room(4 * N), a_bm = room(4 * N * (size_t)M);
    char* block = (char*)c.scratch(need);
    if ((rc = c.begin())) return rc;
    if (!block) return c.error() ? c.error() : fail(HPMVS_ERR_HIP, who + ": out of device memory");
    unsigned int* ctl = (unsigned int*)(block + a_ctl);
    uint8_t *state = (uint8_t*)(block + a_state), *ok = (uint8_t*)(block + a_ok), *sub = (uint8_t*)(block + a_sub), *node_event = (uint8_t*)(block + a_nev);
    uint32_t *mark = (uint32_t*)(block + a_mark), *scan = (uint32_t*)(block + a_scan);
    int32_t *node_of = (int32_t*)(block + a_node), *item_of = (int32_t*)(block + a_item), *slot_of = (int32_t*)(block + a_slot), *rows = (int32_t*)(block + a_rows);
    uint32_t *flow_off = (uint32_t*)(block + a_foff), *anti_off = (uint32_t*)(block + a_aoff);
    DevBatch B;   // the compact batch: the nodes for the graph, then each wave's pending refined candidates for the gates
    memset(&B, 0, sizeof(B));
    B.max_images = M;
    B.center = (float*)(block + a_bc); B.normal = (float*)(block + a_bn); B.scale = (float*)(block + a_bs);
    B.n_images = (int32_t*)(block + a_bi); B.images = (int32_t*)(block + a_bm);
    auto temp_of = [&c](size_t bytes) { return c.scratch(bytes ? bytes : 16); };
#define WALK_PRIM(call_with_temp)                                                                        \
    do {                                                                                                 \
        void* temp = nullptr; size_t temp_bytes = 0;                                                     \
        if ((call_with_temp) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM size query failed");      \
        if (!(temp = temp_of(temp_bytes))) return c.error();                                             \
        if ((call_with_temp) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM call failed");            \
    } while (0)

    // 1. the flags, before anything is written
    HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
    launch_walk_check(n, dflags, dset, ctl + 8, st);
    unsigned int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, ctl + 8, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail(HPMVS_ERR_ARG, who + ": " + std::to_string(bad) + " items with a flag byte that cannot occur (an event that is refined or border, an unknown bit) or a negative set");
    // 2. the nodes in queue order and the graph over them
    launch_walk_mark(n, dflags, mark, st);
    WALK_PRIM(walk_scan(temp, &temp_bytes, mark, scan, n, st));
    launch_walk_nodes(n, dflags, mark, scan, node_of, item_of, node_event, sub, ctl + 9, st);
    unsigned int n_nodes = 0;
    HIPCHK(hipMemcpyAsync(&n_nodes, ctl + 9, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_nodes > (unsigned int)n) return fail(HPMVS_ERR_HIP, who + ": node count");
    uint32_t *flow_adj = nullptr, *anti_adj = nullptr;
    if (n_nodes) {
        B.n = (int)n_nodes;
        launch_walk_gather(D, item_of, (int)n_nodes, B, st);
        int32_t* fp = (int32_t*)c.scratch(4 * (size_t)n_nodes * (11 * (size_t)M + 3 * (size_t)V));
        if (!fp) return c.error();
        conflicts::Footprints F;
        F.n = (int)n_nodes; F.M = M; F.V = V; F.n_levels = n_levels; F.n_images = B.n_images; F.is_event = node_event;
        int32_t *wr = fp, *fr = wr + (size_t)n_nodes * M * 4, *at = fr + (size_t)n_nodes * M * 4, *vb = at + (size_t)n_nodes * M * 3;
        F.wr = wr; F.fr = fr; F.at = at; F.vb = vb;
        launch_depth_footprints(dev_scene(s), s->ddepth, B, wr, fr, at, vb, st);
        HIPCHK(hipGetLastError());
        const unsigned long long* pairs = nullptr;
        uint32_t nf = 0, na = 0;
        const int grc = launch_conflicts(F, [&c](size_t bytes) { return c.scratch(bytes); }, flow_off, anti_off, &pairs, &nf, &na, st);
        if (grc == kConflictsMemory) return c.error() ? c.error() : fail(HPMVS_ERR_HIP, who + ": out of device memory");
        if (grc == kConflictsTooMany)
            return fail(HPMVS_ERR_STATE, who + ": more than 2^30 conflicting (reader, writer) pairs before duplicates are dropped");
        if (grc != kConflictsOk) return fail(HPMVS_ERR_HIP, who + ": " + hipGetErrorString(hipGetLastError()));
        flow_adj = (uint32_t*)c.scratch(4 * ((size_t)nf + 1)); anti_adj = (uint32_t*)c.scratch(4 * ((size_t)na + 1));
        if (!flow_adj || !anti_adj) return c.error();
        launch_conflicts_adjacency(pairs, nf, na, flow_adj, anti_adj, st);
        HIPCHK(hipGetLastError());
    }
    // 3. the key records, sorted by (set, key, item): two stable sorts
    unsigned long long *k0 = (unsigned long long*)(block + a_k0), *k1 = (unsigned long long*)(block + a_k1), *rec_key = (unsigned long long*)(block + a_key);
    uint32_t *v0 = (uint32_t*)(block + a_v0), *v1 = (uint32_t*)(block + a_v1), *rec_val = (uint32_t*)(block + a_val);
    uint32_t *s0 = (uint32_t*)(block + a_s0), *rec_set = (uint32_t*)(block + a_set), *p0 = (uint32_t*)(block + a_p0), *perm = (uint32_t*)(block + a_perm);
    launch_walk_records(n, dflags, dpre, dpost, k0, v0, st);
    WALK_PRIM(walk_sort_keys64(temp, &temp_bytes, k0, k1, v0, v1, 2 * n, st));
    launch_walk_record_sets(n, dflags, dset, v1, s0, p0, st);
    WALK_PRIM(walk_sort_keys32(temp, &temp_bytes, s0, rec_set, p0, perm, 2 * n, st));
    launch_walk_permute(n, perm, k1, v1, rec_key, rec_val, st);
    level_walk::Level L;
    L.n = n; L.min_images = o->MIN_IMAGES_PER_PATCH; L.flags = dflags; L.set = dset; L.pre = dpre; L.post = dpost;
    L.node_of = node_of; L.item_of = item_of; L.flow_off = flow_off; L.flow_adj = flow_adj; L.anti_off = anti_off; L.anti_adj = anti_adj;
    L.n_rec = 2u * (unsigned int)n; L.rec_set = rec_set; L.rec_key = rec_key; L.rec_val = rec_val;
    L.first_pre = (uint32_t*)(block + a_fpre); L.first_post = (uint32_t*)(block + a_fpost);
    launch_walk_first(L, (uint32_t*)(block + a_fpre), (uint32_t*)(block + a_fpost), st);
    // 4. the waves.  From here on the outputs and the maps are written.
    launch_walk_init(n, state, ok, dcounts, daccepted, dwave, st);
    HIPCHK(hipGetLastError());
    WalkArrays A;
    A.state = state; A.ok = ok; A.slot_of = slot_of; A.gv = (int32_t*)(block + a_gv); A.gb = (int32_t*)(block + a_gb); A.gf = (int32_t*)(block + a_gf);
    A.n_images = D.n_images; A.stage = dstage; A.counts = dcounts; A.wave = dwave; A.accepted = daccepted;
    DevBatch Dok = D;   // the level's batch with this wave's accepted / applied items as its ok mask: rows in queue order
    Dok.ok = ok;
    const DevScene sc = dev_scene(s);
    unsigned long long *op_keys = nullptr, *op_sorted = nullptr;
    void* op_temp = nullptr;
    size_t op_temp_bytes = 0;
    int waves = 0, rounds_all = 0, rounds_most = 0, finishes = 0;
    for (int w = 1;; w++) {
        HIPCHK(hipMemsetAsync(ctl, 0, 32, st));
        launch_walk_begin(n, dflags, state, ok, rows, slot_of, ctl, st);
        unsigned int head[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(head, ctl, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const unsigned int pending = head[0], gated = head[1];
        if (!pending) break;
        if (w > n || pending > (unsigned int)n || gated > pending) return fail(HPMVS_ERR_STATE, who + ": the waves do not end (a bug: the first pending item of a wave always decides)");
        waves = w;
        if (gated) {
            B.n = (int)gated;
            launch_walk_gather(D, rows, (int)gated, B, st);
            launch_depth_gates(sc, s->ddepth, B, margin, abs_int, A.gv, A.gb, A.gf, st);
        }
        unsigned int tail[3] = {0, 0, 0};   // ctl[2 .. 4]
        int rounds = 0;
        for (unsigned int decided = 0; decided < pending;) {
            launch_walk_round(L, A, w, ctl, st);
            HIPCHK(hipMemcpyAsync(tail, ctl + 2, 12, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            rounds++;
            if (tail[0] <= decided || tail[0] > pending) return fail(HPMVS_ERR_STATE, who + ": a round decided nothing (a bug: the first undecided item always decides)");
            const bool few = tail[0] - decided < (unsigned int)kWalkFewDecided;
            decided = tail[0];
            if (few && decided < pending && pending - decided <= (unsigned int)kWalkFinishBudget) {   // the end of a chain: one wavefront takes the rest in order
                launch_walk_finish(L, A, w, kWalkFinishBudget, ctl, st);
                HIPCHK(hipMemcpyAsync(tail, ctl + 2, 12, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                finishes++;
                if (tail[0] <= decided || tail[0] > pending) return fail(HPMVS_ERR_STATE, who + ": the in-order pass decided nothing (a bug)");
                decided = tail[0];
            }
        }
        HIPCHK(hipGetLastError());
        rounds_all += rounds; rounds_most = std::max(rounds_most, rounds);
        if (tail[1] && !tail[2]) launch_set_depths(sc, s->ddepth, Dok, st);   // additions only: a minimum per cell, any order
        else if (tail[1]) {
            const size_t cap = N * (size_t)M;
            if (!op_keys) {
                op_keys = (unsigned long long*)c.scratch(8 * cap); op_sorted = (unsigned long long*)c.scratch(8 * cap);
                if (!op_keys || !op_sorted) return c.error();
            }
            HIPCHK(hipMemsetAsync(ctl + 10, 0, 4, st));
            launch_depth_ops_keys(sc, s->ddepth, s->depth_pool, Dok, op_keys, ctl + 10, st);
            unsigned int count = 0;
            HIPCHK(hipMemcpyAsync(&count, ctl + 10, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (count > cap) return fail(HPMVS_ERR_HIP, who + ": depth-op key count");
            if (count) {
                size_t bytes = 0;
                if (depth_ops_sort(nullptr, &bytes, op_keys, op_sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM size query failed");
                if (bytes > op_temp_bytes || !op_temp) {
                    if (!(op_temp = temp_of(bytes))) return c.error();
                    op_temp_bytes = bytes;
                }
                if (depth_ops_sort(op_temp, &bytes, op_keys, op_sorted, count, st) != 0) return fail(HPMVS_ERR_HIP, who + ": rocPRIM sort failed");
                launch_depth_ops_apply(sc, s->ddepth, s->depth_pool, Dok, sub, op_sorted, count, st);
            }
        }
        HIPCHK(hipGetLastError());
    }
#undef WALK_PRIM
    *n_waves = waves;
    s->last_walk[0] = rounds_all; s->last_walk[1] = rounds_most; s->last_walk[2] = finishes;
    return c.finish();   // (waits in both forms: the scratch is freed on return)
}
// rounds of the last hpmvs_level_walk_batch on this scene, the most in one wave, and its in-order passes
int hpmvs_last_level_walk(const hpmvs_scene* s, int32_t* rounds, int32_t* most_rounds, int32_t* in_order_passes) {
    if (!s) return fail(HPMVS_ERR_ARG, "last_level_walk: null scene");
    if (rounds) *rounds = s->last_walk[0];
    if (most_rounds) *most_rounds = s->last_walk[1];
    if (in_order_passes) *in_order_passes = s->last_walk[2];
    return HPMVS_OK;
}

// how many patches of the last refinement launch outgrew the batch kernel's 64-id rows and were redone by the wide kernel
int hpmvs_last_wide_patches(const hpmvs_scene* s, int32_t* n) {
    if (!s || !n) return fail(HPMVS_ERR_ARG, "last_wide_patches: null argument");
    *n = 0;
    if (!s->last_ws) return HPMVS_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n, s->last_ws + 241, sizeof(int32_t), hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

// debug: phase counters of the last optimize launch (only meaningful in -DHPMVS_PROFILE_PHASES builds)
int hpmvs_debug_counters(const hpmvs_scene* s, unsigned long long* out4) {
    if (!s || !out4) return fail(HPMVS_ERR_ARG, "debug_counters: null argument");
    HIPCHK(hipSetDevice(s->device));
    { const int rcq = service_quiesce(s); if (rcq) return rcq; }
    HIPCHK(hipDeviceSynchronize());
    if (!s->last_queue) return fail(HPMVS_ERR_STATE, "debug_counters: no launch yet");
    HIPCHK(hipMemcpy(out4, (char*)s->last_queue + 16, 544, hipMemcpyDeviceToHost));
    return HPMVS_OK;
}

// how the arrays of the last host-pointer hpmvs_optimize_batch call of this scene (the path above the small-batch
// thresholds) reached the device: bytes copied through device buffers, bytes used in place (pinned, mapped host memory)
int hpmvs_last_staging(const hpmvs_scene* s, unsigned long long* staged_bytes, unsigned long long* in_place_bytes) {
    if (!s || !staged_bytes || !in_place_bytes) return fail(HPMVS_ERR_ARG, "last_staging: null argument");
    *staged_bytes = s->last_staged_bytes; *in_place_bytes = s->last_mapped_bytes;
    return HPMVS_OK;
}

// pinned host memory mapped into the GPUs' address space, for callers without the HIP headers: arrays of a host-pointer
// call that live in it are used in place (see mapped_host)
void* hpmvs_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void hpmvs_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

int hpmvs_last_kernel_ms(const hpmvs_scene* s, float* ms) {
    if (!s || !ms) return fail(HPMVS_ERR_ARG, "last_kernel_ms: null argument");
    if (!s->timed) return fail(HPMVS_ERR_STATE, "last_kernel_ms: no optimize launch yet");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return HPMVS_OK;
}

}  // extern "C"
