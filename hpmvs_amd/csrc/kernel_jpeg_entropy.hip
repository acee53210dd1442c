// kernel_jpeg_entropy.hip -- the Huffman scan of a baseline JPEG decoded in parallel (jpeg.hpp: decode_subseq and what
// stands around it; restated in loops by tests/jpeg_entropy_host.cpp).  The host's prescan hands over the scan without
// stuffing, cut into segments at the restart markers; every segment is cut into subsequences of S bits, one work-item each.
//   jpeg_entropy_sync_kernel    pass 0 decodes every subsequence from the guess (its first bit, block 0, k 0) and then
//                               re-decodes, round by round, every subsequence whose predecessor's exit is not the entry it
//                               used, inside the workgroup (exits in LDS); a later pass does the same after the workgroup's
//                               first subsequence took the exit of the workgroup before it from the pass before
//   jpeg_entropy_scan_*         inclusive sums of the blocks completed and the DC differences per component (mod 2^32)
//   jpeg_entropy_check_kernel   accepts the chain or not
//   jpeg_entropy_write_kernel   decodes once more from the accepted entries and stores the coefficients where
//                               decode_scan stores them, DC predictions included
// All loops are bounded by the round budget, the subsequence count or a segment's bits (decode_subseq consumes a bit per
// iteration or stops).  Every store is bounded by the array it goes to; coefficient addresses are checked in decode_subseq.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace hpmvs {

namespace {

constexpr int kTabWords = (int)(6 * sizeof(jpg::Huff) / 4);
static_assert(sizeof(jpg::Huff) % 4 == 0, "the tables are copied to LDS in words");
static_assert(jpg::kSubsPerGroup == 64, "one wavefront per workgroup");

// the six tables and the zigzag order behind them: global -> LDS (the caller synchronises)
__device__ void load_tables(const uint32_t* __restrict__ g, uint32_t* s_tabs, uint8_t* s_zz, int tid, int n) {
    for (int k = tid; k < kTabWords; k += n) s_tabs[k] = g[k];
    const uint8_t* zz = reinterpret_cast<const uint8_t*>(g + kTabWords);
    for (int k = tid; k < 64; k += n) s_zz[k] = zz[k];
}

__device__ uint32_t sub_end(const jpg::Segment& g, uint32_t i, uint32_t S) {
    const unsigned long long e = (unsigned long long)(i + 1) * S;
    return e < g.bits ? (uint32_t)e : g.bits;
}

__device__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ uint4 sub4(uint4 a, uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// inclusive sum over the subsequences 0 .. j (j < n_subs)
__device__ uint4 incl_at(const JpegEntropy& A, uint32_t j) { return add4(A.incl[j], A.grp[j >> 8]); }

}  // namespace

__global__ void __launch_bounds__(64) jpeg_entropy_sync_kernel(JpegEntropy A, int pass, int budget) {
    __shared__ uint32_t s_tabs[kTabWords];
    __shared__ uint8_t s_zz[64];
    __shared__ jpg::SubState s_exit[64];
    const int tid = threadIdx.x;
    load_tables(A.tabs, s_tabs, s_zz, tid, 64);
    const jpg::Huff* tabs = reinterpret_cast<const jpg::Huff*>(s_tabs);
    const uint32_t j = blockIdx.x * 64u + (uint32_t)tid;
    const bool live = j < A.n_subs;
    jpg::Segment g = {0, 0, 0, 0, 0, 1};
    if (live) g = A.segs[A.sub_seg[j]];
    const uint32_t i = live ? j - g.first_sub : 0u;
    const uint32_t end = sub_end(g, i, A.subseq_bits);
    const uint8_t* d = A.bytes + g.first_byte;
    const bool first = i == 0;  // of its segment: the entry is no guess
    jpg::SubState entry = {0, 0}, exit = {0, 0};
    jpg::SubCount cnt = {0, {0, 0, 0}};
    __syncthreads();
    if (live) {
        if (pass == 0) {
            entry = jpg::guess_state(i, A.subseq_bits);
            exit = jpg::decode_subseq(d, g.bits, end, tabs, A.si, s_zz, entry, &cnt, nullptr, 0, 0, 0, nullptr);
        } else {
            entry = A.entry[j];
            exit = A.exit[j];
            const uint4 c = A.cnt[j];
            cnt.nblk = c.x; cnt.dc[0] = c.y; cnt.dc[1] = c.z; cnt.dc[2] = c.w;
        }
    }
    int r = 0;
    bool overflow = false;
    for (;;) {
        s_exit[tid] = exit;
        __syncthreads();
        jpg::SubState pred = entry;
        if (live && !first) {
            if (tid > 0) pred = jpg::handed_on(s_exit[tid - 1]);
            else if (pass > 0) pred = A.grp_exit[(size_t)((pass - 1) & 1) * A.n_groups + blockIdx.x - 1];  // (blockIdx.x > 0: not first)
        }
        const bool need = live && !first && !jpg::same_state(pred, entry);
        const int any = __syncthreads_or(need ? 1 : 0);
        if (!any) break;
        if (r == budget) { overflow = true; break; }
        if (need) {
            entry = pred;
            exit = jpg::decode_subseq(d, g.bits, end, tabs, A.si, s_zz, entry, &cnt, nullptr, 0, 0, 0, nullptr);
        }
        r++;
    }
    if (live) {
        A.entry[j] = entry;
        A.exit[j] = exit;
        A.cnt[j] = make_uint4(cnt.nblk, cnt.dc[0], cnt.dc[1], cnt.dc[2]);
    }
    if (tid == 63) A.grp_exit[(size_t)(pass & 1) * A.n_groups + blockIdx.x] = jpg::handed_on(exit);
    if (tid == 0) {
        if (r) atomicMax(&A.flags[0], (uint32_t)r);
        if (overflow) atomicOr(&A.flags[1], 1u);
    }
}

// 256 subsequences per workgroup: inclusive sums inside it, and its total
__global__ void __launch_bounds__(256) jpeg_entropy_scan_local_kernel(JpegEntropy A) {
    __shared__ uint4 s[256];
    const int tid = threadIdx.x;
    const uint32_t j = blockIdx.x * 256u + (uint32_t)tid;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (j < A.n_subs) v = A.cnt[j];
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        uint4 t = make_uint4(0, 0, 0, 0);
        if (tid >= o) t = s[tid - o];
        __syncthreads();
        v = add4(v, t);
        s[tid] = v;
        __syncthreads();
    }
    if (j < A.n_subs) A.incl[j] = v;
    if (tid == 255) A.grp[blockIdx.x] = v;
}

// the workgroups' totals -> what stands in front of each of them; one workgroup walks them 256 at a time
__global__ void __launch_bounds__(256) jpeg_entropy_scan_groups_kernel(JpegEntropy A) {
    __shared__ uint4 s[256];
    const int tid = threadIdx.x;
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (uint32_t base = 0; base < A.n_scan_groups; base += 256) {
        const uint32_t w = base + (uint32_t)tid;
        const uint4 own = w < A.n_scan_groups ? A.grp[w] : make_uint4(0, 0, 0, 0);
        uint4 v = own;
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            uint4 t = make_uint4(0, 0, 0, 0);
            if (tid >= o) t = s[tid - o];
            __syncthreads();
            v = add4(v, t);
            s[tid] = v;
            __syncthreads();
        }
        if (w < A.n_scan_groups) A.grp[w] = add4(carry, sub4(v, own));
        carry = add4(carry, s[255]);
        __syncthreads();
    }
}

// flags[2] != 0 afterwards: the chain is not the sequential decode, or the sequential decode is none the host accepts
__global__ void __launch_bounds__(256) jpeg_entropy_check_kernel(JpegEntropy A) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= A.n_subs) return;
    const uint32_t sg = A.sub_seg[j];
    const jpg::Segment g = A.segs[sg];
    const jpg::SubState entry = A.entry[j], exit = A.exit[j];
    jpg::SubState want = {0, 0};
    if (j != g.first_sub) want = jpg::handed_on(A.exit[j - 1]);
    bool ok = jpg::same_state(entry, want) && !(exit.bk & jpg::kStateErr);
    if (ok && j + 1 == g.first_sub + g.n_subs) {
        uint4 total = incl_at(A, j);
        if (g.first_sub) total = sub4(total, incl_at(A, g.first_sub - 1));
        ok = jpg::segment_ok(g, exit, total.x, A.si.bpm, sg + 1 == A.n_segs);
    }
    if (!ok) atomicOr(&A.flags[2], 1u);
}

__global__ void __launch_bounds__(64) jpeg_entropy_write_kernel(JpegEntropy A, int16_t* __restrict__ coef) {
    __shared__ uint32_t s_tabs[kTabWords];
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x;
    load_tables(A.tabs, s_tabs, s_zz, tid, 64);
    __syncthreads();
    const uint32_t j = blockIdx.x * 64u + (uint32_t)tid;
    if (j >= A.n_subs || A.flags[2]) return;  // (a chain the check refused is not written: the host decodes)
    const jpg::Segment g = A.segs[A.sub_seg[j]];
    const uint32_t i = j - g.first_sub;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 base = g.first_sub ? incl_at(A, g.first_sub - 1) : zero;
    const uint4 before = sub4(j ? incl_at(A, j - 1) : zero, base);
    const uint32_t dc_in[3] = {before.y, before.z, before.w};
    jpg::decode_subseq(A.bytes + g.first_byte, g.bits, sub_end(g, i, A.subseq_bits), reinterpret_cast<const jpg::Huff*>(s_tabs), A.si, s_zz,
                       A.entry[j], nullptr, coef, before.x, g.first_mcu, g.n_mcus * (uint32_t)A.si.bpm, dc_in);
}

void launch_jpeg_entropy_sync(const JpegEntropy& A, int pass, int budget, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(A.n_groups), dim3(64), 0, st, A, pass, budget);
}

hipError_t launch_jpeg_entropy_finish(const JpegEntropy& A, int16_t* coef, hipStream_t st, hipEvent_t* ev) {
    hipError_t e = hipSuccess;
    if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_entropy_scan_local_kernel, dim3(A.n_scan_groups), dim3(256), 0, st, A);
    if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_entropy_scan_groups_kernel, dim3(1), dim3(256), 0, st, A);
    if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_entropy_check_kernel, dim3(A.n_scan_groups), dim3(256), 0, st, A);
    if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3(A.n_groups), dim3(64), 0, st, A, coef);
    if (ev && (e = hipEventRecord(ev[4], st)) != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace hpmvs
