// kernel_conflicts.hip -- an extend level's conflict graph built on the device (include/hpmvs_amd.h: hpmvs_level_conflicts_batch,
// hpmvs_conflicts_from_footprints).  Every rule -- which cells a footprint names, which pair a match gives -- is
// conflicts.hpp's; this file gives them threads.
//
//   conflicts_records_kernel   one thread per (node, image): the write's (cell key, node), compacted with one atomic per wavefront
//   (radix sort of the records by key)
//   conflicts_bound_kernel     one wavefront per node: the records inside its items' key ranges, two bounds per range and no walk --
//                              an upper bound of the pairs, and what the 2^30 limit is held against
//   conflicts_pairs_kernel    one wavefront per node, lanes striding over its items (conflicts.hpp: a candidate's reads, an event's
//                              writes); an item is at most two key ranges, each a lower bound in the sorted keys and a walk to its
//                              end.  EMIT = false counts the pairs; EMIT = true writes them, a wavefront reserving room for 64
//                              items' pairs with one atomic.  Their order does not matter: they are sorted next.
//   (radix sort of the pairs, rocPRIM unique)
//   conflicts_offsets_kernel   one thread per node: its two CSR offsets are lower bounds in the sorted pairs
//   conflicts_adjacency_kernel one thread per pair: the member, into the list the pair's top bit names
//
// Plain global memory throughout: the sorted keys of a level (~1 MB) stay in L2, and no kernel shares data inside a block.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "conflicts.hpp"
#include "launch.h"

namespace hpmvs {

namespace {

using conflicts::Footprints;

__device__ __forceinline__ int cf_lane() { return (int)__lane_id(); }

__global__ void __launch_bounds__(256) conflicts_records_kernel(Footprints F, unsigned long long* __restrict__ keys, uint32_t* __restrict__ nodes,
                                                                unsigned int* __restrict__ counter) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / F.M), k = (int)(t - (long long)i * F.M);
    unsigned long long key = 0ull;
    const bool valid = i < F.n && conflicts::write_key(F, i, k, key);
    const unsigned long long m = __ballot(valid);
    if (m) {
        const int lane = cf_lane(), first = __ffsll((long long)m) - 1;
        unsigned int base = 0;
        if (lane == first) base = atomicAdd(counter, (unsigned int)__popcll(m));
        base = (unsigned int)__builtin_amdgcn_readlane((int)base, first);
        if (valid) {
            const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));   // < n * M: one slot per valid thread
            keys[at] = key; nodes[at] = (uint32_t)i;
        }
    }
}

// the pairs of node i's item q among the sorted records: counted, and with EMIT written from `out` on
template <bool EMIT>
__device__ __forceinline__ unsigned int item_pairs(const Footprints& F, int i, int q, const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ nodes, size_t n_rec, unsigned long long* out) {
    conflicts::Ranges R;
    conflicts::item_ranges(F, i, q, R);
    unsigned int c = 0;
    for (int r = 0; r < R.n; r++)
        for (size_t at = conflicts::lower_bound_key(keys, n_rec, R.lo[r]); at < n_rec && keys[at] <= R.hi[r]; at++) {
            unsigned long long p;
            if (!conflicts::pair_of(F, i, (int)nodes[at], p)) continue;
            if (EMIT) out[c] = p;
            c++;
        }
    return c;
}

// the wavefront's sum of `mine` added to *counter by lane 0
__device__ __forceinline__ void wave_sum_add(unsigned long long mine, unsigned long long* counter) {
    unsigned int lo = (unsigned int)mine, hi = (unsigned int)(mine >> 32);
    unsigned long long sum = mine;
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned int olo = __shfl_down(lo, d, 64), ohi = __shfl_down(hi, d, 64);
        sum += ((unsigned long long)ohi << 32) | olo;
        lo = (unsigned int)sum; hi = (unsigned int)(sum >> 32);
    }
    if (cf_lane() == 0 && sum) atomicAdd(counter, sum);
}

// The level's matches (conflicts.hpp: item_matches), two bounds per key range and no walk: what decides whether the level is
// refused, so that a hostile input -- every node on one cell -- costs O(log) per range and never the walk over its pairs.
__global__ void __launch_bounds__(256) conflicts_bound_kernel(Footprints F, const unsigned long long* __restrict__ keys,
                                                              const unsigned int* __restrict__ n_rec_p, unsigned long long* __restrict__ counter) {
    const int lane = cf_lane();
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const size_t n_rec = (size_t)*n_rec_p;
    unsigned long long mine = 0ull;
    for (int i = wave; i < F.n; i += nwaves) {
        const int items = conflicts::item_count(F, i);
        for (int q = lane; q < items; q += 64) mine += conflicts::item_matches(F, i, q, keys, n_rec);
    }
    wave_sum_add(mine, counter);
}

// `bound_p` (the count pass): the matches conflicts_bound_kernel summed -- beyond the limit nothing is walked, the host refuses
template <bool EMIT>
__global__ void __launch_bounds__(256) conflicts_pairs_kernel(Footprints F, const unsigned long long* __restrict__ keys,
                                                              const uint32_t* __restrict__ nodes, const unsigned int* __restrict__ n_rec_p,
                                                              const unsigned long long* __restrict__ bound_p,
                                                              unsigned long long* __restrict__ counter, unsigned long long* __restrict__ pairs,
                                                              unsigned long long cap) {
    if (!EMIT && *bound_p > conflicts::kMaxRawPairs) return;   // (uniform over the grid)
    const int lane = cf_lane();
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const size_t n_rec = (size_t)*n_rec_p;
    unsigned long long mine = 0ull;   // (the count pass: this lane's pairs over all its nodes)
    for (int i = wave; i < F.n; i += nwaves) {
        const int items = conflicts::item_count(F, i);
        for (int base = 0; base < items; base += 64) {
            const int q = base + lane;
            const unsigned int c = q < items ? item_pairs<false>(F, i, q, keys, nodes, n_rec, nullptr) : 0u;
            if (!EMIT) { mine += c; continue; }
            // room for the 64 items' pairs: an inclusive scan over the lanes, one atomic by the last lane
            unsigned int inc = c;
            for (int d = 1; d < 64; d <<= 1) { const unsigned int up = __shfl_up(inc, d, 64); if (lane >= d) inc += up; }
            const unsigned int total = __shfl(inc, 63, 64);
            if (!total) continue;
            unsigned long long start = 0ull;
            if (lane == 63) start = atomicAdd(counter, (unsigned long long)total);
            const unsigned int lo = __shfl((unsigned int)start, 63, 64), hi = __shfl((unsigned int)(start >> 32), 63, 64);
            const unsigned long long at = (((unsigned long long)hi << 32) | lo) + (inc - c);
            if (c && at + c <= cap) item_pairs<true>(F, i, q, keys, nodes, n_rec, pairs + at);   // (never beyond what the count pass sized)
        }
    }
    if (!EMIT) wave_sum_add(mine, counter);
}

// off[i] for i = 0 .. n; totals[0] = |flow|, totals[1] = |anti|.  `count_p`: the number of unique pairs (rocPRIM wrote it)
__global__ void __launch_bounds__(256) conflicts_offsets_kernel(int n, const unsigned long long* __restrict__ pairs, const unsigned int* __restrict__ count_p,
                                                                uint32_t* __restrict__ flow_off, uint32_t* __restrict__ anti_off,
                                                                uint32_t* __restrict__ totals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const size_t m = (size_t)*count_p;
    const size_t n_flow = conflicts::lower_bound_key(pairs, m, conflicts::kAntiBit);
    const unsigned long long owner = (unsigned long long)(unsigned)i << 32;
    flow_off[i] = (uint32_t)conflicts::lower_bound_key(pairs, m, owner);   // (i == n: every flow pair is below n << 32, every anti pair above)
    anti_off[i] = (uint32_t)(conflicts::lower_bound_key(pairs, m, conflicts::kAntiBit | owner) - n_flow);
    if (i == n) { totals[0] = (uint32_t)n_flow; totals[1] = (uint32_t)(m - n_flow); }
}
__global__ void __launch_bounds__(256) conflicts_adjacency_kernel(const unsigned long long* __restrict__ pairs, unsigned int n_flow, unsigned int n_anti,
                                                                  uint32_t* __restrict__ flow_adj, uint32_t* __restrict__ anti_adj) {
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_flow + n_anti) return;
    if (k < n_flow) flow_adj[k] = (uint32_t)pairs[k];
    else anti_adj[k - n_flow] = (uint32_t)pairs[k];
}

inline unsigned int wave_blocks(int n) {
    int blocks = (n + 3) / 4;   // one wavefront per node, four to a block
    return (unsigned int)(blocks > 256 * 32 ? 256 * 32 : blocks);
}

}  // namespace

// The graph of footprints F (device arrays) up to the sorted, unique pairs and the CSR offsets.  `scratch` gives device memory that
// lives until the caller's call ends (null: out of memory).  Host-synchronous: three counts are read back on the way.
// Returns kConflictsOk, or kConflictsHip (a HIP or rocPRIM call failed), kConflictsMemory, kConflictsTooMany (matches beyond
// conflicts::kMaxRawPairs: nothing written, no pair walked).
int launch_conflicts(const Footprints& F, const std::function<void*(size_t)>& scratch, uint32_t* flow_off, uint32_t* anti_off,
                     const unsigned long long** pairs_out, uint32_t* n_flow, uint32_t* n_anti, hipStream_t st) {
#define CF_HIP(expr) do { if ((expr) != hipSuccess) return kConflictsHip; } while (0)
    const size_t slots = (size_t)F.n * (size_t)F.M;
    // counters: [0] records (u32) | [2..3] raw pairs (u64) | [4..5] emitted (u64) | [6] unique pairs | [8], [9] totals | [10..11] matches (u64)
    uint32_t* cnt = (uint32_t*)scratch(64);
    unsigned long long* keys_in = (unsigned long long*)scratch(8 * slots);
    unsigned long long* keys = (unsigned long long*)scratch(8 * slots);
    uint32_t* nodes_in = (uint32_t*)scratch(4 * slots);
    uint32_t* nodes = (uint32_t*)scratch(4 * slots);
    if (!cnt || !keys_in || !keys || !nodes_in || !nodes) return kConflictsMemory;
    CF_HIP(hipMemsetAsync(cnt, 0, 64, st));
    hipLaunchKernelGGL(conflicts_records_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, F, keys_in, nodes_in, cnt);
    uint32_t n_rec = 0;
    CF_HIP(hipMemcpyAsync(&n_rec, cnt, 4, hipMemcpyDeviceToHost, st));
    CF_HIP(hipStreamSynchronize(st));
    if (n_rec > slots) return kConflictsHip;
    if (n_rec) {
        size_t temp_bytes = 0;
        CF_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys, nodes_in, nodes, (size_t)n_rec, 0u, 64u, st));
        void* temp = scratch(temp_bytes ? temp_bytes : 16);
        if (!temp) return kConflictsMemory;
        CF_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys, nodes_in, nodes, (size_t)n_rec, 0u, 64u, st));
    }
    // the bound, then the exact count -- which walks nothing when the bound is over the limit -- and ONE read-back of the two
    unsigned long long *raw_p = (unsigned long long*)(cnt + 2), *bound_p = (unsigned long long*)(cnt + 10);
    hipLaunchKernelGGL(conflicts_bound_kernel, dim3(wave_blocks(F.n)), dim3(256), 0, st, F, keys, cnt, bound_p);
    hipLaunchKernelGGL(conflicts_pairs_kernel<false>, dim3(wave_blocks(F.n)), dim3(256), 0, st, F, keys, nodes, cnt, bound_p, raw_p,
                       (unsigned long long*)nullptr, 0ull);
    unsigned long long back[5] = {0, 0, 0, 0, 0};   // cnt[2 .. 11]
    CF_HIP(hipMemcpyAsync(back, raw_p, sizeof(back), hipMemcpyDeviceToHost, st));
    CF_HIP(hipStreamSynchronize(st));
    const unsigned long long raw = back[0], bound = back[4];
    if (bound > conflicts::kMaxRawPairs) return kConflictsTooMany;
    if (raw > bound) return kConflictsHip;   // (cannot be: every pair is a match)
    unsigned long long* pairs = nullptr;
    if (raw) {
        unsigned long long* pairs_in = (unsigned long long*)scratch(8 * (size_t)raw);
        unsigned long long* sorted = (unsigned long long*)scratch(8 * (size_t)raw);
        if (!pairs_in || !sorted) return kConflictsMemory;
        hipLaunchKernelGGL(conflicts_pairs_kernel<true>, dim3(wave_blocks(F.n)), dim3(256), 0, st, F, keys, nodes, cnt, bound_p, (unsigned long long*)(cnt + 4), pairs_in, raw);
        size_t temp_bytes = 0;
        if (depth_ops_sort(nullptr, &temp_bytes, pairs_in, sorted, (unsigned int)raw, st) != 0) return kConflictsHip;
        void* temp = scratch(temp_bytes ? temp_bytes : 16);
        if (!temp) return kConflictsMemory;
        if (depth_ops_sort(temp, &temp_bytes, pairs_in, sorted, (unsigned int)raw, st) != 0) return kConflictsHip;
        // duplicates out (eight images of two nodes on one cell are one edge): pairs_in is free again and takes the result
        size_t ubytes = 0;
        CF_HIP(rocprim::unique(nullptr, ubytes, sorted, pairs_in, cnt + 6, (size_t)raw, rocprim::equal_to<unsigned long long>(), st));
        void* utemp = scratch(ubytes ? ubytes : 16);
        if (!utemp) return kConflictsMemory;
        CF_HIP(rocprim::unique(utemp, ubytes, sorted, pairs_in, cnt + 6, (size_t)raw, rocprim::equal_to<unsigned long long>(), st));
        pairs = pairs_in;
    }
    hipLaunchKernelGGL(conflicts_offsets_kernel, dim3((unsigned)((F.n + 1 + 255) / 256)), dim3(256), 0, st, F.n, pairs, cnt + 6, flow_off, anti_off, cnt + 8);
    uint32_t totals[2] = {0, 0};
    CF_HIP(hipMemcpyAsync(totals, cnt + 8, 8, hipMemcpyDeviceToHost, st));
    CF_HIP(hipStreamSynchronize(st));
    CF_HIP(hipGetLastError());
    *pairs_out = pairs; *n_flow = totals[0]; *n_anti = totals[1];
    return kConflictsOk;
#undef CF_HIP
}

void launch_conflicts_adjacency(const unsigned long long* pairs, uint32_t n_flow, uint32_t n_anti, uint32_t* flow_adj, uint32_t* anti_adj, hipStream_t st) {
    const size_t m = (size_t)n_flow + n_anti;
    if (!m) return;
    hipLaunchKernelGGL(conflicts_adjacency_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, pairs, n_flow, n_anti, flow_adj, anti_adj);
}

}  // namespace hpmvs
