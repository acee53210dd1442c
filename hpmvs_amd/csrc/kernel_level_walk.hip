// kernel_level_walk.hip -- the wave walk of an extend level on the device (include/hpmvs_amd.h: hpmvs_level_walk_batch; DESIGN.md
// §3.19).  Every decision is level_walk.hpp's decide(); this file gives it threads.  The graph, the gates and the depth updates are
// the kernels of kernel_conflicts.hip and kernel_depth.hip, launched by the entry point (capi.hip) between these.
//
//   walk_check_kernel       one thread per item: flag bytes that cannot occur and negative sets, counted
//   walk_mark_kernel        one thread per item: is it a node of the graph (an event or a refined candidate)?
//   (rocPRIM exclusive scan of the marks)
//   walk_nodes_kernel       one thread per item: node_of / item_of, the node's event flag, the item's subtract flag
//   walk_gather_kernel      one thread per (row, image slot): the rows of a patch batch that a list names, into a compact batch --
//                           the nodes for the footprint kernel, a wave's pending refined candidates for depth_gates_kernel
//   walk_records_kernel     one thread per (item, role): its key record, (key, item << 1 | role); none: key ~0
//   (stable radix sort by key)   walk_record_sets_kernel: the sorted records' sets (none: kNoSet)   (stable radix sort by set)
//   walk_permute_kernel     the records in (set, key, item) order
//   walk_first_kernel       one thread per item: the first record of its pre key and of its post key -- once per level
//   walk_init_kernel        the outputs' start values: from here on the call writes
//   walk_begin_kernel       one thread per item, once per wave: next_wave_state; the pending items are counted and the refined ones
//                           among them listed (one atomic per wavefront; the gates do not need them in order)
//   walk_round_kernel       one thread per item, once per round: an undecided item decides once no earlier neighbour that can
//                           still change its outcome is undecided.  A thread reads other items' states while other threads write them: a state only ever goes
//                           from undecided to final within a wave, a stale read is "undecided", and the item waits one more round.
//                           No thread waits inside the kernel; the host reads how many decided and launches the next round.
//   walk_finish_kernel      ONE wavefront decides the next undecided items IN ORDER (at most `budget`): what the entry point
//                           launches when a round decided only a few and few are left -- the end of a chain, which rounds would
//                           take one launch per link.  The wavefront looks 64 states at a time; lane 0 decides (every earlier
//                           item is decided by then).
// The accepted and applied items of a wave are not compacted: ok[i] marks them in the level's own batch, whose rows are in queue
// order -- the order the depth-op keys carry (depth_ops_keys_kernel: call index = row).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "launch.h"
#include "level_walk.hpp"

namespace hpmvs {

namespace {

namespace lw = level_walk;

__device__ __forceinline__ int lw_lane() { return (int)__lane_id(); }
// the wavefront's count of `flag` added to *counter by its first lane
__device__ __forceinline__ void lw_count(bool flag, unsigned int* counter) {
    const unsigned long long m = __ballot(flag);
    if (m && lw_lane() == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned int)__popcll(m));
}

__global__ void __launch_bounds__(256) walk_check_kernel(int n, const uint8_t* __restrict__ flags, const int32_t* __restrict__ set,
                                                         unsigned int* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    lw_count(i < n && (!lw::flags_valid(flags[i]) || (set && set[i] < 0)), bad);
}
__global__ void __launch_bounds__(256) walk_mark_kernel(int n, const uint8_t* __restrict__ flags, uint32_t* __restrict__ mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mark[i] = lw::is_node(flags[i]) ? 1u : 0u;
}
// n_nodes[0]: the number of nodes
__global__ void __launch_bounds__(256) walk_nodes_kernel(int n, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ mark,
                                                         const uint32_t* __restrict__ scan, int32_t* __restrict__ node_of,
                                                         int32_t* __restrict__ item_of, uint8_t* __restrict__ node_event,
                                                         uint8_t* __restrict__ subtract, unsigned int* __restrict__ n_nodes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ev = lw::is_event(flags[i]);
    subtract[i] = ev ? 1 : 0;
    if (mark[i]) { node_of[i] = (int32_t)scan[i]; item_of[scan[i]] = i; node_event[scan[i]] = ev ? 1 : 0; }   // (scan[i] < n)
    else node_of[i] = -1;
    if (i == n - 1) *n_nodes = scan[i] + mark[i];
}

__global__ void __launch_bounds__(256) walk_gather_kernel(DevBatch src, const int32_t* __restrict__ rows, int count, DevBatch dst) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M = src.max_images;
    const int r = (int)(t / M), k = (int)(t - (long long)r * M);
    if (r >= count) return;
    const int i = rows[r];   // (a row of src: the lists hold item indices below src.n)
    dst.images[(size_t)r * M + k] = src.images[(size_t)i * M + k];
    if (k < 4) { dst.center[4 * r + k] = src.center[4 * i + k]; dst.normal[4 * r + k] = src.normal[4 * i + k]; }
    if (k == 0) { dst.scale[r] = src.scale[i]; dst.n_images[r] = src.n_images[i]; }
    if (M < 4 && k == 0)
        for (int q = M; q < 4; q++) { dst.center[4 * r + q] = src.center[4 * i + q]; dst.normal[4 * r + q] = src.normal[4 * i + q]; }
}

__global__ void __launch_bounds__(256) walk_records_kernel(int n, const uint8_t* __restrict__ flags, const unsigned long long* __restrict__ pre,
                                                           const unsigned long long* __restrict__ post, unsigned long long* __restrict__ key,
                                                           uint32_t* __restrict__ val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;   // record r = item << 1 | role, r < 2 n
    if (r >= 2 * n) return;
    const int i = r >> 1;
    const bool on = (r & 1) ? lw::has_post_record(flags[i]) : lw::has_pre_record(flags[i]);
    key[r] = on ? ((r & 1) ? post[i] : pre[i]) : ~0ull;
    val[r] = (uint32_t)r;
}
__global__ void __launch_bounds__(256) walk_record_sets_kernel(int n, const uint8_t* __restrict__ flags, const int32_t* __restrict__ set,
                                                               const uint32_t* __restrict__ val, uint32_t* __restrict__ rec_set,
                                                               uint32_t* __restrict__ pos) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2 * n) return;
    const uint32_t v = val[r];
    const int i = (int)(v >> 1);
    const bool on = (v & 1u) ? lw::has_post_record(flags[i]) : lw::has_pre_record(flags[i]);
    rec_set[r] = on ? (set ? (uint32_t)set[i] : 0u) : lw::kNoSet;
    pos[r] = (uint32_t)r;
}
__global__ void __launch_bounds__(256) walk_permute_kernel(int n, const uint32_t* __restrict__ perm, const unsigned long long* __restrict__ key_in,
                                                           const uint32_t* __restrict__ val_in, unsigned long long* __restrict__ key,
                                                           uint32_t* __restrict__ val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2 * n) return;
    key[r] = key_in[perm[r]]; val[r] = val_in[perm[r]];   // (perm: a permutation of 0 .. 2 n - 1)
}
__global__ void __launch_bounds__(256) walk_first_kernel(lw::Level L, uint32_t* __restrict__ first_pre, uint32_t* __restrict__ first_post) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t set = lw::set_of(L, i);
    first_pre[i] = lw::first_record(L.rec_set, L.rec_key, L.n_rec, set, L.pre[i]);
    first_post[i] = lw::first_record(L.rec_set, L.rec_key, L.n_rec, set, L.post[i]);
}

__global__ void __launch_bounds__(256) walk_init_kernel(int n, uint8_t* __restrict__ state, uint8_t* __restrict__ ok, int32_t* __restrict__ counts,
                                                        uint8_t* __restrict__ accepted, int32_t* __restrict__ wave) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    state[i] = lw::kUndecided; ok[i] = 0; accepted[i] = 0; wave[i] = 0;
    counts[3 * i] = counts[3 * i + 1] = counts[3 * i + 2] = -1;
}

// ctl[0]: pending items, ctl[1]: the refined candidates among them (rows[] / slot_of[])
__global__ void __launch_bounds__(256) walk_begin_kernel(int n, const uint8_t* __restrict__ flags, uint8_t* __restrict__ state,
                                                         uint8_t* __restrict__ ok, int32_t* __restrict__ rows, int32_t* __restrict__ slot_of,
                                                         unsigned int* __restrict__ ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool pending = false, gated = false;
    if (i < n) {
        const uint8_t s = lw::next_wave_state(state[i]);
        state[i] = s; ok[i] = 0;
        pending = s == lw::kUndecided;
        gated = pending && !lw::is_event(flags[i]) && (flags[i] & lw::kRefined);
    }
    lw_count(pending, ctl);
    const unsigned long long m = __ballot(gated);
    if (m) {
        const int lane = lw_lane(), first = __ffsll((long long)m) - 1;
        unsigned int base = 0;
        if (lane == first) base = atomicAdd(ctl + 1, (unsigned int)__popcll(m));
        base = (unsigned int)__builtin_amdgcn_readlane((int)base, first);
        if (gated) {
            const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));   // < n: one slot per refined candidate
            rows[at] = i; slot_of[i] = (int32_t)at;
        }
    }
}

struct WalkOut {
    uint8_t *state, *ok;               // ok: this wave's accepted / applied items, the mask of the depth update
    const int32_t *slot_of, *gv, *gb, *gf, *n_images;
    int32_t *stage, *counts, *wave;
    uint8_t* accepted;
};
// item i, undecided: decided if it can be.  0: it waits, 1: decided, 3: decided and an op of the wave, 7: ... a subtraction
__device__ __forceinline__ int walk_decide(const lw::Level& L, const WalkOut& W, int i, int w) {
    const uint8_t fl = L.flags[i];
    const bool gated = !lw::is_event(fl) && (fl & lw::kRefined);
    int v = 0, b = 0, f = 0, nimg = 1;
    if (gated) { const int k = W.slot_of[i]; v = W.gv[k]; b = W.gb[k]; f = W.gf[k]; nimg = W.n_images[i]; }
    lw::Outcome o;
    if (!lw::decide(L, W.state, i, v, b, f, nimg, o)) return 0;
    if (o.stage >= 0) W.stage[i] = o.stage;
    W.counts[3 * i] = o.counts ? v : -1; W.counts[3 * i + 1] = o.counts ? b : -1; W.counts[3 * i + 2] = o.counts ? f : -1;
    W.wave[i] = w;
    const bool op = o.state == lw::kAccept || o.state == lw::kApply;
    if (o.state == lw::kAccept) W.accepted[i] = 1;
    if (op) W.ok[i] = 1;
    W.state[i] = o.state;
    return 1 | (op ? 2 : 0) | (o.state == lw::kApply ? 4 : 0);
}
// ctl[2]: items decided in this wave, ctl[3]: its ops, ctl[4]: the subtractions among them
__global__ void __launch_bounds__(256) walk_round_kernel(lw::Level L, WalkOut W, int w, unsigned int* __restrict__ ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (i < L.n && W.state[i] == lw::kUndecided) ? walk_decide(L, W, i, w) : 0;
    lw_count(r & 1, ctl + 2); lw_count(r & 2, ctl + 3); lw_count(r & 4, ctl + 4);
}
__global__ void __launch_bounds__(64) walk_finish_kernel(lw::Level L, WalkOut W, int w, int budget, unsigned int* __restrict__ ctl) {
    const int lane = lw_lane();
    unsigned int decided = 0, ops = 0, subs = 0;   // (lane 0's)
    bool stop = false;
    for (int base = 0; base < L.n && !stop; base += 64) {
        const int i = base + lane;
        unsigned long long m = __ballot(i < L.n && W.state[i] == lw::kUndecided);
        while (m && !stop) {
            const int at = base + __ffsll((long long)m) - 1;
            m &= m - 1;
            int r = 0;
            if (lane == 0) {
                r = walk_decide(L, W, at, w);   // (every earlier item is decided: it decides; if not, the entry point sees no progress)
                decided += r & 1; ops += (r >> 1) & 1; subs += (r >> 2) & 1;
            }
            r = __builtin_amdgcn_readfirstlane(r);
            stop = !(r & 1) || (int)__builtin_amdgcn_readfirstlane((int)decided) >= budget;
        }
    }
    if (lane == 0) { atomicAdd(ctl + 2, decided); atomicAdd(ctl + 3, ops); atomicAdd(ctl + 4, subs); }
}

inline unsigned int blocks_of(size_t threads) { return (unsigned int)((threads + 255) / 256); }

}  // namespace

void launch_walk_check(int n, const uint8_t* flags, const int32_t* set, unsigned int* bad, hipStream_t st) {
    hipLaunchKernelGGL(walk_check_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, st, n, flags, set, bad);
}
// temp == nullptr: only reports the temporary bytes rocPRIM needs
int walk_scan(void* temp, size_t* temp_bytes, const uint32_t* in, uint32_t* out, int n, hipStream_t st) {
    return (int)rocprim::exclusive_scan(temp, *temp_bytes, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
}
void launch_walk_mark(int n, const uint8_t* flags, uint32_t* mark, hipStream_t st) {
    hipLaunchKernelGGL(walk_mark_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, st, n, flags, mark);
}
void launch_walk_nodes(int n, const uint8_t* flags, const uint32_t* mark, const uint32_t* scan, int32_t* node_of, int32_t* item_of,
                       uint8_t* node_event, uint8_t* subtract, unsigned int* n_nodes, hipStream_t st) {
    hipLaunchKernelGGL(walk_nodes_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, st, n, flags, mark, scan, node_of, item_of, node_event,
                       subtract, n_nodes);
}
void launch_walk_gather(const DevBatch& src, const int32_t* rows, int count, const DevBatch& dst, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(walk_gather_kernel, dim3(blocks_of((size_t)count * (size_t)src.max_images)), dim3(256), 0, st, src, rows, count, dst);
}
int walk_sort_keys64(void* temp, size_t* temp_bytes, const unsigned long long* key_in, unsigned long long* key, const uint32_t* val_in,
                     uint32_t* val, int count, hipStream_t st) {
    return (int)rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key, val_in, val, (size_t)count, 0u, 64u, st);
}
int walk_sort_keys32(void* temp, size_t* temp_bytes, const uint32_t* key_in, uint32_t* key, const uint32_t* val_in, uint32_t* val, int count,
                     hipStream_t st) {
    return (int)rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key, val_in, val, (size_t)count, 0u, 32u, st);
}
void launch_walk_records(int n, const uint8_t* flags, const unsigned long long* pre, const unsigned long long* post, unsigned long long* key,
                         uint32_t* val, hipStream_t st) {
    hipLaunchKernelGGL(walk_records_kernel, dim3(blocks_of(2 * (size_t)n)), dim3(256), 0, st, n, flags, pre, post, key, val);
}
void launch_walk_record_sets(int n, const uint8_t* flags, const int32_t* set, const uint32_t* val, uint32_t* rec_set, uint32_t* pos,
                             hipStream_t st) {
    hipLaunchKernelGGL(walk_record_sets_kernel, dim3(blocks_of(2 * (size_t)n)), dim3(256), 0, st, n, flags, set, val, rec_set, pos);
}
void launch_walk_permute(int n, const uint32_t* perm, const unsigned long long* key_in, const uint32_t* val_in, unsigned long long* key,
                         uint32_t* val, hipStream_t st) {
    hipLaunchKernelGGL(walk_permute_kernel, dim3(blocks_of(2 * (size_t)n)), dim3(256), 0, st, n, perm, key_in, val_in, key, val);
}
void launch_walk_first(const level_walk::Level& L, uint32_t* first_pre, uint32_t* first_post, hipStream_t st) {
    hipLaunchKernelGGL(walk_first_kernel, dim3(blocks_of((size_t)L.n)), dim3(256), 0, st, L, first_pre, first_post);
}
void launch_walk_init(int n, uint8_t* state, uint8_t* ok, int32_t* counts, uint8_t* accepted, int32_t* wave, hipStream_t st) {
    hipLaunchKernelGGL(walk_init_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, st, n, state, ok, counts, accepted, wave);
}
void launch_walk_begin(int n, const uint8_t* flags, uint8_t* state, uint8_t* ok, int32_t* rows, int32_t* slot_of, unsigned int* ctl, hipStream_t st) {
    hipLaunchKernelGGL(walk_begin_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, st, n, flags, state, ok, rows, slot_of, ctl);
}
void launch_walk_round(const level_walk::Level& L, const WalkArrays& A, int w, unsigned int* ctl, hipStream_t st) {
    const WalkOut W = {A.state, A.ok, A.slot_of, A.gv, A.gb, A.gf, A.n_images, A.stage, A.counts, A.wave, A.accepted};
    hipLaunchKernelGGL(walk_round_kernel, dim3(blocks_of((size_t)L.n)), dim3(256), 0, st, L, W, w, ctl);
}
void launch_walk_finish(const level_walk::Level& L, const WalkArrays& A, int w, int budget, unsigned int* ctl, hipStream_t st) {
    const WalkOut W = {A.state, A.ok, A.slot_of, A.gv, A.gb, A.gf, A.n_images, A.stage, A.counts, A.wave, A.accepted};
    hipLaunchKernelGGL(walk_finish_kernel, dim3(1), dim3(64), 0, st, L, W, w, budget, ctl);
}

}  // namespace hpmvs
