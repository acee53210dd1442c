// capi_common.hpp -- what the translation units of the C ABI share (capi.hip: the scene and the batch entry points;
// capi_image.hip: the image entry points): the error string and its macros, the device prologue, one owner for a device
// buffer, one accumulator for a working buffer's layout, one set of event marks, the few image functions the scene
// entries of capi.hip call, and the accessor through which capi_image.hip reaches a scene's depth maps.  Host-only; no kernel
// includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/hpmvs_amd.h"
#include "dev_types.h"
#include "jpeg.hpp"
#include "jpeg_enc.hpp"

namespace hpmvs {
namespace capi {

inline size_t reg_align(size_t v) { return (v + 255) & ~(size_t)255; }  // regions of a workspace or a scratch block start at multiples of 256 bytes

extern thread_local std::string g_err;  // behind hpmvs_last_error (capi.hip)

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(HPMVS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

// The prologue of every entry that takes a device index: HPMVS_ERR_NODEVICE without a device, HPMVS_ERR_ARG
// "<who>: bad device index" for one out of range, then the device is the calling thread's current one.
inline int use_device(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(HPMVS_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(HPMVS_ERR_ARG, std::string(who) + ": bad device index");
    HIPCHK(hipSetDevice(device));
    return HPMVS_OK;
}

// A device allocation that lives as long as its owner: freed in the destructor, handed on by move or release().
struct DeviceBuffer {
    uint8_t* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.release()) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { reset(); }
    // (a caller for whom no memory is no error of the call still clears the runtime's sticky error with hipGetLastError)
    hipError_t alloc(size_t bytes) { reset(); const hipError_t e = hipMalloc((void**)&p, bytes); if (e != hipSuccess) p = nullptr; return e; }
    void reset() { if (p) hipFree(p); p = nullptr; }
    uint8_t* release() { uint8_t* q = p; p = nullptr; return q; }
    explicit operator bool() const { return p != nullptr; }
};

// The arrays of one working buffer, each at a 256-byte aligned offset (reg_align); total: the bytes to allocate.
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t at = total; total += reg_align(bytes); return at; }
};

// n HIP events for the stage times a diagnostic entry reports, on the null stream.  on = false (the caller passed no ms
// array): no event exists and every member returns hipSuccess without doing anything.
class EventMarks {
    std::vector<hipEvent_t> ev_;
    hipError_t created_ = hipSuccess;

public:
    EventMarks(int n, bool on) : ev_(on ? (size_t)n : 0, nullptr) {
        for (size_t k = 0; k < ev_.size() && created_ == hipSuccess; k++) created_ = hipEventCreate(&ev_[k]);
    }
    ~EventMarks() { for (hipEvent_t e : ev_) if (e) hipEventDestroy(e); }
    EventMarks(const EventMarks&) = delete;
    EventMarks& operator=(const EventMarks&) = delete;
    hipError_t created() const { return created_; }
    hipError_t mark(int k) { return ev_.empty() ? hipSuccess : hipEventRecord(ev_[k], nullptr); }
    hipError_t sync(int k) { return ev_.empty() ? hipSuccess : hipEventSynchronize(ev_[k]); }
    hipError_t elapsed(int a, int b, float* ms) { return ev_.empty() ? hipSuccess : hipEventElapsedTime(ms, ev_[a], ev_[b]); }
    hipEvent_t* from(int k) { return ev_.empty() ? nullptr : ev_.data() + k; }  // for a launcher that records events k, k + 1, .. itself
};

// ---- the image code (capi_image.hip) as the scene entries of capi.hip see it -------------------------------------------------

// Image::undistort's parameters (reference Image.h:80: float f_, k1_): k1 finite, f finite and positive
inline bool undistort_args_ok(float f, float k1) { return std::isfinite(k1) && std::isfinite(f) && f > 0.0f; }

inline int jpeg_enc_fail(int code, const std::string& msg) { return fail(code == jpge::kErrUnsupported ? HPMVS_ERR_UNSUPPORTED : HPMVS_ERR_ARG, msg); }

// A JPEG file from its bytes (the caller's, which outlive it) to its coefficients.  jpeg_open fills the frame, the eight Huffman
// tables and where the scan starts; jpeg_decode_scan then leaves the coefficients either in fr.coef (the host walked the scan)
// or in d_coef behind the quantiser steps' room, on the current device (kernel_jpeg_entropy.hip decoded it).  d_coef is this
// object's own: whoever declares a JpegFile frees the buffer by leaving its scope, on every path.
struct JpegFile {
    const uint8_t* bytes = nullptr;
    size_t n = 0, scan_start = 0;
    jpg::Frame fr;
    std::vector<jpg::Huff> huff;
    DeviceBuffer d_coef;
    int used = HPMVS_JPEG_ENTROPY_HOST, rounds = 0;
};

// the headers parsed; a refusal as the file's own code (HPMVS_ERR_ARG / _UNSUPPORTED) and message.  Pure host code.
int jpeg_open(const uint8_t* bytes, size_t n, JpegFile& jf);
// The scan of an opened file decoded where `entropy` says, on the current device.  strict: the caller asked for the device
// itself, so what the device does not take is HPMVS_ERR_STATE instead of the host walk.  ms: jpeg_entropy_device's.
int jpeg_decode_scan(JpegFile& jf, int entropy, bool strict, uint32_t subseq_bits = jpg::kSubseqBits, float* ms = nullptr);
int jpeg_frame_to_device(const JpegFile& jf, uint8_t* d_rgb, float* ms = nullptr);
int jpeg_encode_device(const uint8_t* d_rgb, int W, int H, int quality, uint8_t* out, size_t cap, size_t* n, float* ms = nullptr);
int jpeg_entropy_env();
bool jpeg_entropy_ok(int e);

// ---- a scene's depth maps (capi.hip, which alone knows hpmvs_scene) as the depth-image entries of capi_image.hip see them ----
struct SceneDepthMaps {
    int device = 0, n_levels = 0;
    DevDepthView maps = {};  // one view's level pointers and shapes
};
// level: 0 .. n_levels - 1 or HPMVS_DEPTH_COMBINED.  The codes and messages of the depth-map entries: HPMVS_ERR_STATE
// "<who>: call hpmvs_scene_depth_reset first", HPMVS_ERR_ARG "<who>: bad view / level".  Touches no device.
int scene_depth_maps(const hpmvs_scene* s, int view, int level, const char* who, SceneDepthMaps* out);

}  // namespace capi
}  // namespace hpmvs
