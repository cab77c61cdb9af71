// mirsha_ctx.h — internal state shared by the host-side translation units of
// the C-ABI (include/mirsha.h); not part of the ABI.
//
//   mirsha_api.hip      contexts, timing, device-pointer API, synthetic
//                       streams, clock probe
//   mirsha_staging.hip  synchronous host calls: staging, pipelined H2D /
//                       kernels / D2H (mirsha_hash_batch / _slices /
//                       _requests_then_batches, mirsha_digest_lists) and their
//                       verify forms (mirsha_verify_batch / _slices /
//                       _digest_lists: compare on the device, verdict back)
//   mirsha_plan.hip     request -> batch plans: sequential, fused (placement
//                       probe), overlapped cycles (mirsha_pipeline_*)
//   mirsha_async.hip    the asynchronous ring: the slot lifecycle every ticket
//                       kind shares (ring_acquire -> stage / queue ->
//                       ring_publish -> async_complete; RingQueued for a
//                       submission that fails after it queued work) and the
//                       hashing tickets (mirsha_submit_* / wait / poll, dedup,
//                       mixed hash-and-verify cycles: *_expect, both in one
//                       ticket: *_expect_dedup)
//   mirsha_expect.hip   the select kernels of the mixed submissions
//   mirsha_chains.hip   checkpoint chains: every mirsha_chains_* entry point (a
//                       cycle's Commits as a ticket of that ring among them)
//                       and the SHA-256 chain kernels (mirsha_chains.h)
//   mirsha_order.hip    the kernels of the device-built bucket order
//                       (mirsha_order.h; queue_bucket_order in mirsha_api.hip)
//   mirsha_streams.hip  streaming hash states over any bytes (mirsha_streams_*)
//                       and their kernel (mirsha_streams.h)
//   mirsha_streams_ring.hip  a stream programme as a ticket of that ring
//                       (mirsha_streams_submit*) and its segment kernel
//   mirsha_host.cpp     host-only logic, no HIP (dedup scan, packing, the
//                       expectation / commit / stream plans, a mixed ticket's kept-rows
//                       walk): unit-tested on the CPU (tests/c)
//   mirsha_multi.hip    the multi-device drop-in (mirsha_multi_*)
//   mirsha_sha512.hip   the request and list kernels of the second hasher,
//                       SHA-512/256 (mirsha_sha512.h; hasher_launch_* below)
//   mirsha_sha512_chains.hip  its checkpoint-chain kernels
//                       (mirsha_sha512_chains.h; chain_kernels, mirsha_chains.h)
//   mirsha_sha512_streams.hip  its stream kernels
//                       (mirsha_sha512_streams.h; stream_kernels, mirsha_streams.h)
//   mirsha_sha512_plan.hip  its device-plan kernels: the plan-form list walk
//                       and the overlapped cycle (mirsha_sha512_plan.h;
//                       plan_kernels, mirsha_plan.hip)
//   mirsha_sha512_pair.hip  its producer/consumer pair kernels for small
//                       launches and the routed launchers that choose between
//                       them and the one-lane kernels (mirsha_sha512_pair.h;
//                       hasher_launch_* below, plan_kernels)
//   mirsha_sha512_chains_pair.hip  the pair forms of its chains' commit
//                       kernels and their routed launchers
//                       (mirsha_sha512_chains.h; chain_kernels)
//
// Every entry point returns digests in ORIGIN order (processor.go:139 indexes
// Digests[i] by the request's position), unlike ProcessorWorkPool's
// completion-order collector (processor.go:349-356).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mirsha.h"
#include "mirsha_host.h"
#include "mirsha_device.h"
#include "mirsha_order.h"
#include "mirsha_sha512.h"
#include "mirsha_sha512_pair.h"
#include "mirsha_sha512_plan.h"

namespace mirsha {
// mirsha_expect.hip.  Mixed cycles (mirsha_submit_*_expect): compares the
// digests of the requests marked in has[] (ceil(n / 64) words, base[] = set
// bits before each word: mirsha_expect_plan) with their rows of `expected`,
// stores the digest rows of every request without an expectation and of every
// mismatch to row i of `out` (all arrays 16-byte aligned), writes every word
// of the mismatch bitmap; *count += mismatches (the caller resets it on the
// stream first).
hipError_t launch_expect_select(const uint8_t* digests, const uint8_t* expected, const uint64_t* has,
                                const uint32_t* base, uint32_t n, uint8_t* out, uint64_t* bits, uint32_t* count,
                                hipStream_t s);
// The same over a deduplicated cycle (mirsha_submit_slices_expect_dedup):
// request i's digest is row row_of[i] (< m, the caller checked) of the
// representatives' digests, rows [0, m0) in digests0 and [m0, m) in digests1
// (may be NULL when m0 = m).
hipError_t launch_expect_select_gather(const uint8_t* digests0, const uint8_t* digests1, uint32_t m0,
                                       const uint32_t* row_of, const uint8_t* expected, const uint64_t* has,
                                       const uint32_t* base, uint32_t n, uint8_t* out, uint64_t* bits,
                                       uint32_t* count, hipStream_t s);
}  // namespace mirsha

namespace mirsha_api {

constexpr uint64_t kStageChunk = 32ull << 20;  // pinned staging chunk for pageable request bytes
constexpr int kStageSlots = 3;                  // chunks in flight (packed while earlier ones DMA)
constexpr uint64_t kInlineArena = 1ull << 20;   // arenas up to this ride in the metadata copy
constexpr uint64_t kPinnedOutMax = 8ull << 20;  // digest results up to this come back via pinned staging

constexpr uint64_t kArenaSlack = 256;           // loader may touch up to 80 B past a message
constexpr uint32_t kFusedMaxListWaves = 64;      // list groups (64 chains each) a fused launch takes
constexpr uint32_t kFusedMaxListBlocks = 32;     // list CUs (one producer / consumer pair each)
constexpr uint32_t kFusedMinChainBlocks = 64;    // AUTO picks the fused launch from this chain length
constexpr uint32_t kFusedDefaultPace = 4;        // tile waves (= tile queues) per SIMD
constexpr uint32_t kFusedDefaultListTiles = 1;   // FusedArgs::list_tiles (fused_build; profiles/r02au, r02av)

// Grow-only buffers.  A growth frees (hipFree / hipHostFree synchronise the
// device: every queued copy and kernel of every stream must finish first),
// so a buffer grows to 1.5x its old capacity, not to the exact request: ring
// slots see chunks a few hundred bytes apart, and exact-fit growth cost a
// ~9 ms device drain inside a submission now and then (profiles/r05w).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        size_t want = std::max(n, cap + cap / 2);
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipMalloc(&p, n);
            if (e != hipSuccess) { p = nullptr; return e; }
            want = n;
        }
        cap = want;
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        size_t want = std::max(n, cap + cap / 2);
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipHostMalloc(&p, n, hipHostMallocDefault);
            if (e != hipSuccess) { p = nullptr; return e; }
            want = n;
        }
        cap = want;
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// One in-flight submission of the asynchronous API (mirsha_submit_slices):
// its own pinned staging and device buffers, so up to kAsyncSlots Ready()
// cycles can be packed / copied / hashed while the caller works on.
constexpr uint32_t kAsyncSlots = 4;
using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// The expectation side of a mixed submission (mirsha_submit_*_expect).
struct ExpectSlot {
    uint32_t words = 0;   // ceil(n / 64)
    uint64_t o_exp = 0, o_ver = 0, h2d = 0;  // offsets of the expected rows and the verdict; bytes of `stage`
    uint64_t o_row = 0;  // offset of row_of u32[n] (a deduplicated mixed submission), behind the expected rows
    PinnedBuf stage;    // [has u64[words] | base u32[words], padded to 16 | expected 32 m | row_of]: H2D source
    PinnedBuf verdict;  // [count u32, pad | mismatch bitmap u64[words]]: D2H target
    DevBuf dev;         // stage's layout, then the verdict's (16-byte aligned)
};

// A commit submission (mirsha_chains_commit_submit*) or a stream submission
// (mirsha_streams_submit*): the ring slot's own copies of everything the device
// reads, so the caller's arrays are free when the call returns.  A slot carries
// one ticket at a time, so the two kinds share the buffers.
struct CommitSlot {
    // commit: [seg_chain | sfirst | seg_flags | ent | pad to 16 | host digest table]
    // stream: [seg_stream | sfirst | seg_flags | pad to 16 | entry records | packed bytes (host form)]
    PinnedBuf stage;  // ONE H2D
    DevBuf dev;       // the same layout
    DevBuf snap;      // the states as the launch found them: [h | pend | cnt] (commit), the rows (stream)
    PinnedBuf rows;   // the values' rows when values_out is not kernel-writable
};

// What a ticket owes its caller when it retires (async_complete): how its rows
// reach `out`, and which verdict goes to `bits` / `count`.  ring_acquire resets
// it, the submitter fills it in before ring_publish.
enum class SlotRows : uint8_t {
    kInPlace,  // already there: a kernel or a DMA wrote the caller's memory
    kCopyAll,  // rows [0, n) of the slot's `dig`
    kFanOut,   // row rank[i] of `dig` for request i (dedup)
    kKept,     // a mixed ticket's kept rows, from `dig` (mirsha::host::copy_kept_rows)
    kCommit,   // n values from cm.rows: a commit ticket's checkpoints, a stream ticket's sums
};
enum class SlotVerdict : uint8_t {
    kNone,
    kAllZero,  // a mixed ticket without expectations (m == 0): nothing differs
    kDevice,   // count and bitmap from xp.verdict
};
struct SlotRetire {
    SlotRows rows = SlotRows::kInPlace;
    SlotVerdict verdict = SlotVerdict::kNone;
    uint8_t* out = nullptr;  // digests_out / values_out
    uint32_t n = 0;          // its rows: requests, or checkpoint / sum values
    uint64_t* bits = nullptr;  // bits_out (may be NULL) and n_mismatch_out of a ticket that owes a verdict
    uint32_t* count = nullptr;
};

struct AsyncSlot {
    PinnedBuf stage;  // [arena bytes | off u64[m] | len u32[m] | order u32[m]]
    Clock::time_point t_queued;  // when its device work was queued
    PinnedBuf dig;    // m x 32 digests (D2H target)
    DevBuf dev;       // the same layout as stage, then m x 32 digests
    PinnedBuf stage2;  // a dedup submission's second launch (representatives
    DevBuf dev2;       // found after the first), queued behind the first
    hipEvent_t done = nullptr;
    hipEvent_t ev_in = nullptr, ev_kern = nullptr;  // arena submissions: H2D landed, kernel done
    uint64_t ticket = 0;
    bool busy = false;
    SlotRetire retire;
    std::vector<uint32_t> rank;  // request -> row of `dig` (SlotRows::kFanOut; grow-only)
    double prof[MIRSHA_PROF_PHASES] = {};  // this submission's host phases (published when it completes)
    ExpectSlot xp;
    CommitSlot cm;
};

constexpr int kKernelTimers = 10;  // timing ids 0-9 (mirsha.h, mirsha_ctx_kernel_time)
constexpr int kTimerVerify = 6;
constexpr int kTimerExpect = 7;
constexpr int kTimerOrder = 8;
constexpr int kTimerStreams = 9;

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<hipEvent_t> pool;
    uint64_t launches = 0;
    double ms = 0.0;
};


}  // namespace mirsha_api
using namespace mirsha_api;

struct mirsha_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    int variant = mirsha::kVariantLds;
    int hasher = MIRSHA_HASHER_SHA256;  // mirsha_ctx_set_hasher: which kernels hasher_launch_* queue
    // SHA-512/256 launches that took the producer/consumer pair kernels
    // (mirsha_ctx_sha512_pair_launches); counted where a launch is queued, which
    // holds the context const.
    mutable uint64_t sha512_pair_launches = 0;
    bool timing = false;
    uint32_t time_mask = 0xFFFFFFFFu;  // kernels timed while timing is on
    std::string err;
    DevBuf d_arena, d_off, d_len, d_order, d_out, d_idx, d_first, d_out2, d_scratch;
    DevBuf d_scan;  // scratch of the offsets scan (pipelined gapless calls) and of the order's counts scan
    // The device-built bucket order (queue_bucket_order): the mode of the arena
    // submissions, and the counts and their scan, used on c->stream only.
    int order_mode = MIRSHA_ORDER_HOST;
    DevBuf d_order_counts;
    // Staged host calls (see "staged host calls" below): a ring of pinned
    // chunks for pageable request bytes, one pinned metadata block (plus small
    // arenas) -> one H2D, and pinned digest staging for small results.
    PinnedBuf h_ring[kStageSlots];
    hipEvent_t ring_ev[kStageSlots] = {};
    bool ring_busy[kStageSlots] = {};
    PinnedBuf h_meta, h_outs;
    DevBuf d_meta;
    // Pipelined staged calls (run_pipelined): H2D and D2H each on their own
    // stream, so chunk k's digests return while chunk k+1's bytes go in.
    hipStream_t xin = nullptr, xout = nullptr;
    std::vector<hipEvent_t> xev;  // per-call events (grow-only pool)
    // Host scratch of the synchronous slice call (request lengths, packed
    // offsets), kept across calls: fresh vectors cost ~1-2 ms of page faults
    // and zeroing per 2^20 requests.
    std::vector<uint32_t> sl_len;
    std::vector<uint64_t> sl_poff;
    KernelTimer timers[kKernelTimers];  // msgs, lists, gen, chain, fused, overlap, verify, expect, order, streams
    // Verify calls (mirsha_verify_*): the expected digests (pinned staging of a
    // pageable caller array, device copy) and the verdict block
    // [count u32, pad | bitmap u64[ceil(n/64)]] on the device and pinned.
    PinnedBuf h_expect, h_verdict;
    DevBuf d_expect, d_verdict;
    AsyncSlot slots[kAsyncSlots];
    std::vector<uint64_t> xp_has;   // mirsha_expect_plan of the submission being validated
    std::vector<uint32_t> xp_base;
    hipStream_t xcommit = nullptr;  // commit and stream submissions (created at the first one)
    std::vector<uint32_t> cm_plan;  // mirsha_commit_seg_plan of the submission being validated
    uint64_t next_ticket = 1;  // ticket of the next submission
    uint64_t done_ticket = 0;  // every ticket <= this one has completed
    double prof[MIRSHA_PROF_PHASES] = {};  // host phases of the last slice submission (ms)
};

// The last segment ticket (a commit or a stream submission) queued on a state
// object: the object's synchronous calls make their stream wait for it
// (owner_order), its destroy waits for it (owner_retire).
struct RingOwner {
    hipEvent_t ev = nullptr;
    bool queued = false;
};

// Streaming checkpoint chains (see mirsha.h, mirsha_chains_create).
struct mirsha_chains {
    int device = 0;
    uint32_t n = 0;
    int hasher = MIRSHA_HASHER_SHA256;  // fixed at creation: its row of chain_kernels (mirsha_chains.h)
    // state: h / pend / cnt of 32n / 32n / 8n bytes (SHA-256), 64n / 96n / 8n (SHA-512/256)
    DevBuf d_h, d_pend, d_cnt;
    DevBuf d_dig, d_pos, d_act, d_afirst, d_which, d_out;  // per call
    // mirsha_chains_commit: mirsha_commit_plan's arrays in one block
    // [act | efirst | ent], one H2D copy (kept across calls).
    std::vector<uint32_t> plan;
    DevBuf d_plan;
    RingOwner ring;  // mirsha_chains_commit_submit*
    // Commit launches (calls and tickets, absorb included) that took the
    // SHA-512/256 pair kernels (mirsha_chains_pair_launches); counted where a
    // launch is queued.  Stays 0 for SHA-256 chains.
    uint64_t pair_launches = 0;
};

// Streaming hash states (see mirsha.h, mirsha_streams_create).
struct mirsha_streams {
    int device = 0;
    uint32_t n = 0;
    int hasher = MIRSHA_HASHER_SHA256;  // fixed at creation: its row of stream_kernels (mirsha_streams.h)
    uint32_t row_bytes = 0;             // that row's: a stream's row on the device
    DevBuf d_state;  // row_bytes per stream (mirsha_streams.h, mirsha_sha512_streams.h)
    // mirsha_stream_plan's arrays of the call being run or submitted, and
    // mirsha_stream_seg_plan's of a submission (kept across calls)
    std::vector<uint32_t> act, efirst, kind, len;
    std::vector<uint64_t> off, poff;
    std::vector<uint32_t> seg_stream, sfirst, seg_flags;
    // mirsha_streams_run's block [act | efirst | pad to 16 | entries {kind, len,
    // off lo, off hi} | the written bytes, each distinct range once (host
    // form)]: ONE H2D copy.
    PinnedBuf stage;
    DevBuf dev, d_out;
    RingOwner ring;  // mirsha_streams_submit*
};

// A request -> batch-digest pipeline plan (see mirsha.h, mirsha_pipeline_create).
struct mirsha_pipeline {
    int device = 0;
    int mode = MIRSHA_PIPELINE_FUSED;
    int hasher = MIRSHA_HASHER_SHA256;  // fixed at creation (mirsha_pipeline_create_hasher): plan_kernels' case
    uint32_t n_req = 0, n_lists = 0, n_entries = 0;
    // fused mode (one persistent launch, see mirsha_kernels.hip)
    std::vector<uint32_t> tadj_first, tadj, cbase, expected;
    uint32_t n_tiles = 0, n_groups = 0, n_counters = 0, grid = 0;
    uint32_t pace = 1, list_blocks = 0, tile_waves = 0;  // tile waves per SIMD; list blocks first in the grid
    uint32_t list_tiles = 0;  // FusedArgs::list_tiles
    uint32_t q_first[mirsha::kFusedMaxQueues + 1] = {};  // tile queues (fused_build)
    uint32_t q_end[mirsha::kFusedMaxQueues] = {};        // queue q = [q_first[q], q_end[q])
    uint32_t q_waves[mirsha::kFusedMaxQueues] = {};      // waves of each queue's slot
    uint32_t tile_blocks = 0;
    uint64_t epoch = 0;  // completed runs of a fused plan
    DevBuf d_tadj_first, d_tadj, d_cbase, d_expected, d_counters, d_ctl, d_trace;
    // Sticky error word of a fused plan, in host-mapped memory: the launch's
    // list waves set it on a readiness-watchdog expiry; every later call on the
    // plan reads it without a synchronisation and fails (fail closed).
    unsigned long long* h_err = nullptr;
    unsigned long long* d_err = nullptr;
    unsigned long long watchdog = mirsha::kFusedWatchdogTicks;
    // split tiles (FusedArgs::n_split)
    uint32_t n_split = 0, split_first = 0, seg_per_tile = 0, seg_nominal_nb = 0;
    std::vector<uint32_t> seg_nb;
    DevBuf d_seg_nb, d_seg_state, d_seg_flags;
    uint64_t seg_runs = 0;  // launches of the plan (segment flags are monotone over them)
    // Fused plans probe the block placement at creation (launch_placement_probe):
    // not cyclic -> the plan is built SEQUENTIAL instead (fallback = 1).
    int fallback = 0;
    uint32_t test_placement = 0;  // FusedArgs::test_placement (tests only)
    DevBuf d_probe;
    bool trace = false;
    std::vector<uint32_t> cidx, cfirst;      // compacted lists (no null entries)
    uint32_t uniform = 0;                    // B: identity lists of B entries (uniform_lists), else 0
    // Every length given at creation equal: what the request launch may assume
    // of each tile until the tile's own lengths and offsets say otherwise
    // (mirsha_hints.h; packed requests, stride = length).  valid == 0: none.
    mirsha::UniformHint hint{};
    std::vector<uint32_t> order;             // request processing order
    DevBuf d_cidx, d_cfirst, d_order;
};

namespace mirsha_api {

int fail(mirsha_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                    \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail((c), _e == hipErrorOutOfMemory ? MIRSHA_ENOMEM : MIRSHA_EHIP,       \
                        "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

hipEvent_t take_event(KernelTimer& t);

// One launch (a launch function that launches at most one kernel), timed
// when timing is on for `which`: the two events ride on the kernel's own
// dispatch (mirsha::launch_k, hipExtLaunchKernel), so they carry its start
// and end timestamps and add no marker packets to the stream.
template <class F>
int timed_launch(mirsha_ctx* c, int which, F&& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = c->timing && ((c->time_mask >> which) & 1u);
    if (timed) {
        e0 = take_event(c->timers[which]);
        e1 = take_event(c->timers[which]);
        if (e0 && e1) mirsha::next_launch_events() = {e0, e1};
    }
    hipError_t e = launch();
    // unconsumed: the launch function launched nothing (an empty call)
    const bool bound = e0 && e1 && !mirsha::next_launch_events().start;
    mirsha::next_launch_events() = {};
    if (timed && (!bound || e != hipSuccess)) {
        if (e0) c->timers[which].pool.push_back(e0);
        if (e1) c->timers[which].pool.push_back(e1);
    }
    if (e != hipSuccess) return fail(c, MIRSHA_EHIP, "kernel launch: %s", hipGetErrorString(e));
    if (bound) c->timers[which].pending.emplace_back(e0, e1);
    return MIRSHA_OK;
}

// The context's hasher (mirsha_ctx_set_hasher) decides which kernel a hashing
// launch queues; the callers pass what launch_msgs / launch_lists take and
// know nothing else about hashers.  Timing ids 0 and 1 are by role (request
// kernel, list kernel), so the callers keep them.  Under SHA-512/256 the
// routed launchers (mirsha_sha512_pair.h) pick the pair or the one-lane kernel
// by the launch's size and the context's variant, one kernel either way.
inline hipError_t hasher_launch_msgs(const mirsha_ctx* c, const uint8_t* arena, uint64_t arena_len,
                                     const uint64_t* off, const uint32_t* len, const uint32_t* order, uint32_t n,
                                     uint8_t* out, hipStream_t s, const mirsha::UniformHint* hint = nullptr) {
    if (c->hasher == MIRSHA_HASHER_SHA512_256)
        return mirsha::launch_sha512_msgs(arena, arena_len, off, len, order, n, out, c->variant, s,
                                          &c->sha512_pair_launches);
    return mirsha::launch_msgs(arena, arena_len, off, len, order, n, out, c->variant, s, hint);
}
inline hipError_t hasher_launch_lists(const mirsha_ctx* c, const uint8_t* digests, uint32_t n_digests,
                                      const uint32_t* idx, uint32_t n_entries, const uint32_t* first, uint32_t n_lists,
                                      uint32_t* scratch, uint8_t* out, hipStream_t s) {
    if (c->hasher == MIRSHA_HASHER_SHA512_256)
        return mirsha::launch_sha512_lists(digests, n_digests, idx, n_entries, first, n_lists, scratch, out, s,
                                           &c->sha512_pair_launches);
    return mirsha::launch_lists(digests, n_digests, idx, n_entries, first, n_lists, scratch, out, s);
}

inline const char* hasher_name(int hasher) { return hasher == MIRSHA_HASHER_SHA512_256 ? "sha512_256" : "sha256"; }

// The entry guard of a call that is built for SHA-256 only (the two older
// create calls of the device plans, mirsha_pipeline_create / _create_mode):
// refused under any other hasher, ahead of any other effect.
inline int sha256_only(mirsha_ctx* c, const char* call) {
    if (!c || c->hasher == MIRSHA_HASHER_SHA256) return MIRSHA_OK;  // (a NULL context is the call's own MIRSHA_EINVAL)
    return fail(c, MIRSHA_EINVAL, "%s: hasher %s is not built for this call", call, hasher_name(c->hasher));
}

// The entry guard of a hashing call on checkpoint chains: served when the
// context hashes with the chains' own function, else refused ahead of any
// other effect (a log that hashes with another function than the requests is
// a misconfiguration).
inline int chains_hasher_match(mirsha_ctx* c, const mirsha_chains* ch, const char* call) {
    if (!c || !ch || c->hasher == ch->hasher) return MIRSHA_OK;  // (NULL is the call's own MIRSHA_EINVAL)
    return fail(c, MIRSHA_EINVAL, "%s: the chains hash with %s, the context with %s", call, hasher_name(ch->hasher),
                hasher_name(c->hasher));
}

// The same for the two run calls of a device plan
// (mirsha_hash_requests_then_batches_device, mirsha_pipeline_overlap_device)
// and the plan's own hasher.
inline int plan_hasher_match(mirsha_ctx* c, const mirsha_pipeline* p, const char* call) {
    if (!c || !p || c->hasher == p->hasher) return MIRSHA_OK;  // (NULL is the call's own MIRSHA_EINVAL)
    return fail(c, MIRSHA_EINVAL, "%s: the plan hashes with %s, the context with %s", call, hasher_name(p->hasher),
                hasher_name(c->hasher));
}

// The same for the six stream calls (run, run_device, submit, submit_device,
// export, import) and the streams' own hasher.
inline int streams_hasher_match(mirsha_ctx* c, const mirsha_streams* st, const char* call) {
    if (!c || !st || c->hasher == st->hasher) return MIRSHA_OK;  // (NULL is the call's own MIRSHA_EINVAL)
    return fail(c, MIRSHA_EINVAL, "%s: the streams hash with %s, the context with %s", call, hasher_name(st->hasher),
                hasher_name(c->hasher));
}

int use_device(mirsha_ctx* c);

inline uint32_t host_blocks(uint32_t L) { return (uint32_t)(((uint64_t)L + 72u) >> 6); }

// Stable sort of message indices by block count, longest first; true if the
// order is the identity (one bucket).
bool bucket_order(const uint32_t* len, uint32_t n, uint32_t* order);

// The device-built bucket order (mirsha_order.h) of d_len[0, n) with block
// counts in [bmin, bmax], bmin < bmax, at most MIRSHA_ORDER_MAX_BINS bins.
// order_buffers sizes the context's scratch (it may free and so drain the
// device: before a submission queues anything); queue_bucket_order then only
// queues, on c->stream: count (timing id 8), scan, scatter (id 8).
struct OrderShape {
    uint32_t bmax = 0, bins = 0, chunk = 0, n_chunks = 0;
    size_t scan_bytes = 0;
};
int order_buffers(mirsha_ctx* c, uint32_t n, uint32_t bmin, uint32_t bmax, OrderShape* shape);
int queue_bucket_order(mirsha_ctx* c, const OrderShape& shape, const uint32_t* d_len, uint32_t n, uint32_t* d_order);

// Orders the context's stream behind the object's last queued segment ticket
// (no host wait); nothing to do when there was none.
inline int owner_order(mirsha_ctx* c, const RingOwner& o) {
    if (!o.queued) return MIRSHA_OK;
    HIP_TRY(c, hipStreamWaitEvent(c->stream, o.ev, 0));
    return MIRSHA_OK;
}

// An object's destroy: its last queued segment ticket still uses the state.
inline void owner_retire(RingOwner& o) {
    if (!o.ev) return;
    (void)hipEventSynchronize(o.ev);
    (void)hipEventDestroy(o.ev);
    o = RingOwner{};
}

// The issue priority of the segment kernels' waves (seg_prio, mirsha_device.h).
// MIRSHA_AB=1 MIRSHA_COMMIT_PRIO=n (0-3) is the A/B knob of both.  3 was
// measured for the commit wave only; the stream wave takes
// it unmeasured.
constexpr uint32_t kCommitSegPrio = 3;
inline uint32_t commit_seg_prio() {
    const char* e = mirsha::ab_getenv("MIRSHA_COMMIT_PRIO");
    if (e && e[0] >= '0' && e[0] <= '3' && e[1] == 0) return (uint32_t)(e[0] - '0');
    return kCommitSegPrio;
}

int check_lists(mirsha_ctx* c, const uint32_t* idx, const uint32_t* first, uint32_t n_lists, uint32_t n_digests);

// Queues the device compare of n digests on c->stream: the count word is
// reset (a memset on the stream), then verify_digests_kernel (timing id 6)
// writes every word of the bitmap and adds up the mismatches.  n == 0: the
// reset only.
int queue_verify(mirsha_ctx* c, const uint8_t* d_digests, const uint8_t* d_expected, uint32_t n, uint64_t* d_bits,
                 uint32_t* d_count);

// A boolean A/B or diagnostic knob ("1" = set; only with MIRSHA_AB=1).
inline bool getenv_flag(const char* name) {
    const char* e = mirsha::ab_getenv(name);
    return e && e[0] == '1';
}

inline bool host_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Page-locked host memory a kernel on `device` may store into: allocated or
// registered with that device current, or portable (every device maps it).
// Anything else takes the D2H path.
inline bool kernel_writable_host(const void* p, int device) {
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && (a.device == device || (a.allocationFlags & hipHostMallocPortable));
}

constexpr uint64_t align8(uint64_t x) { return (x + 7u) & ~7ull; }
constexpr uint64_t align16(uint64_t x) { return (x + 15u) & ~15ull; }

// ---- mirsha_staging.hip
// The bytes to hash, as the packed arena [0, total).
struct ArenaSrc {
    const uint8_t* base = nullptr;        // contiguous: arena byte x = base[x]; or
    const uint8_t* const* ptr = nullptr;  // slice lists: request i = its slices, at poff[i]
    const uint64_t* slen = nullptr;
    const uint32_t* sfirst = nullptr;
    const uint64_t* poff = nullptr;
    uint32_t n = 0;
    uint64_t total = 0;
};
// `layout`: kInOrder = the messages lie in [0, total) in index order (each
// starts at or after the previous one's end), which the pipelined form needs;
// kGapless = in order with no gaps (off[i] - shift = len[0] + ... + len[i-1]).
enum ArenaLayout { kAnyOrder = 0, kInOrder = 1, kGapless = 2 };
// A verify call (mirsha_verify_*): the staged call keeps its digests on the
// device, compares them there with `expected` (32 bytes each: the n request
// digests, or with lists the n_lists list digests) and brings back only the
// verdict; req_out / list_out are unused (NULL).
struct VerifyArgs {
    const uint8_t* expected = nullptr;
    uint64_t* bits_out = nullptr;  // ceil(count / 64) words, or NULL
    uint32_t* n_mismatch_out = nullptr;
};
int run_staged(mirsha_ctx* c, const ArenaSrc& src, const uint64_t* off, const uint32_t* len, uint32_t n,
               uint64_t shift, ArenaLayout layout, const uint32_t* idx, const uint32_t* first, uint32_t n_lists,
               uint8_t* req_out, uint8_t* list_out, const VerifyArgs* verify = nullptr);
int arena_span(mirsha_ctx* c, uint64_t arena_len, const uint64_t* off, const uint32_t* len, uint32_t n,
               uint64_t* lo_out, uint64_t* hi_out, uint64_t* total_out = nullptr, ArenaLayout* layout_out = nullptr);
int run_arena_call(mirsha_ctx* c, const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                   uint32_t n, const uint32_t* idx, const uint32_t* first, uint32_t n_lists, uint8_t* req_out,
                   uint8_t* list_out, const VerifyArgs* verify = nullptr);
int slice_errors(mirsha_ctx* c, const uint8_t* err, uint32_t n);
int slice_args(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len, const uint32_t* slice_first,
               uint32_t n, const uint8_t* out);
int slice_lengths(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                  const uint32_t* slice_first, uint32_t n, const uint8_t* out, std::vector<uint32_t>& len);

// ---- mirsha_async.hip
// Retires every submission up to `ticket`, in ticket order.
int async_wait_upto(mirsha_ctx* c, uint64_t ticket);

// The life of a ring slot, the same for every kind of ticket ("The
// ring"): ring_acquire -> the submitter stages, queues its device work with
// sl.done behind it and fills sl.retire in -> ring_publish -> async_complete.
// A submission that fails before ring_publish consumes no ticket; the device
// work it had queued still reads the slot's buffers, so it is drained (RingQueued).

// The slot the next ticket takes: makes the device current, retires the slot's
// previous ticket if it is still busy, resets sl.retire, makes sure of sl.done.
int ring_acquire(mirsha_ctx* c, AsyncSlot** slot);
int ensure_event(mirsha_ctx* c, hipEvent_t* e);  // creates *e (no timing) unless it exists

// The streams a submission queues device work on: arm() before the first
// queued operation, ring_publish disarms; still armed at the end of the
// submitter (every exit with an error), it synchronises them.
struct RingQueued {
    hipStream_t s[3];
    bool armed = false;
    explicit RingQueued(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr) : s{a, b, c} {}
    RingQueued(const RingQueued&) = delete;
    ~RingQueued() {
        for (hipStream_t q : s)
            if (armed && q) (void)hipStreamSynchronize(q);
    }
    void arm() { armed = true; }
};

// The one place a ticket is handed out: the slot is busy with the next ticket,
// keeps the submission's host phases ph[], and *ticket_out is written.
void ring_publish(mirsha_ctx* c, AsyncSlot& sl, RingQueued& queued, const double* ph, uint64_t* ticket_out);

// Caller memory a kernel on the context's device may store 128-bit rows into
// (page-locked for that device or portable, 16-byte aligned): its device
// alias, else NULL.
uint8_t* host_rows(mirsha_ctx* c, void* p);
// A slot's own page-locked rows, as a kernel addresses them.
int pinned_rows(mirsha_ctx* c, const PinnedBuf& b, uint8_t** rows);

// A segment ticket: a commit or a stream submission after its checks and its
// plan (a call refused there has left the ring as it was).  What the two kinds
// differ in, beside the callables of seg_submit:
struct SegTicket {
    RingOwner* owner = nullptr;
    bool on_device = false;               // the device form: the input is read behind c->stream
    const uint32_t* seg_flags = nullptr;  // the plan's, n_seg of them (0: nothing to queue)
    uint32_t n_seg = 0;
    uint64_t stage_bytes = 0;  // cm.stage's block: the ONE H2D
    uint64_t dev_slack = 0;    // bytes of cm.dev behind the block
    struct {
        void* p;
        uint64_t bytes;
    } state[3] = {};           // the owner's state arrays: copied to cm.snap when a FIRST lane may not read them in place
    uint8_t* values_out = nullptr;
    uint32_t values = 0;
    int timer = 0;  // the launch's timing id
};

// The slot lifecycle of a segment ticket, t0 = when the submitter began its
// checks.  fill(stage) writes the staging block; launch(dev, state_in, rows, q)
// launches the segment kernel on q: dev = the block on the device, state_in[k]
// = state[k] or its snapshot, rows = where the values go.  Every ensure() lies
// ahead of anything queued (a growth frees and so drains the device); a failure
// after the first queued operation drains the commit stream (RingQueued).
template <class Fill, class Launch>
int seg_submit(mirsha_ctx* c, const SegTicket& t, Clock::time_point t0, Fill fill, Launch launch,
               uint32_t* n_values_out, uint64_t* ticket_out) {
    double ph[MIRSHA_PROF_PHASES] = {};
    ph[MIRSHA_PROF_VALIDATE] = ms_since(t0);
    t0 = Clock::now();
    AsyncSlot* slot = nullptr;
    if (int rc = ring_acquire(c, &slot)) return rc;
    AsyncSlot& sl = *slot;
    CommitSlot& cm = sl.cm;
    if (t.n_seg) {
        if (!c->xcommit) HIP_TRY(c, hipStreamCreateWithFlags(&c->xcommit, hipStreamNonBlocking));
        if (int rc = ensure_event(c, &t.owner->ev)) return rc;
        if (t.on_device)
            if (int rc = ensure_event(c, &sl.ev_in)) return rc;
    }
    RingQueued queued(c->xcommit);
    bool straddle = false;
    uint8_t* rows = nullptr;
    if (t.n_seg) {
        straddle = mirsha::host::seg_straddle(t.seg_flags, t.n_seg, 64);
        HIP_TRY(c, cm.stage.ensure(t.stage_bytes));
        HIP_TRY(c, cm.dev.ensure(t.stage_bytes + t.dev_slack));
        if (straddle) HIP_TRY(c, cm.snap.ensure(t.state[0].bytes + t.state[1].bytes + t.state[2].bytes));
        if (t.values) {
            // a kernel-writable values_out receives the values from the kernel
            // itself, else the slot's rows do, copied out at retirement
            rows = host_rows(c, t.values_out);
            if (!rows) {
                HIP_TRY(c, cm.rows.ensure(32ull * t.values));
                if (int rc = pinned_rows(c, cm.rows, &rows)) return rc;
                sl.retire.rows = SlotRows::kCommit;
                sl.retire.out = t.values_out;
                sl.retire.n = t.values;
            }
        }
    }
    ph[MIRSHA_PROF_PLAN] = ms_since(t0);
    t0 = Clock::now();
    auto queue = [&]() -> int {
        fill(cm.stage.as<uint8_t>());
        hipStream_t q = c->xcommit;
        queued.arm();
        if (t.on_device) {  // the input is read behind whatever was queued on the context's stream
            HIP_TRY(c, hipEventRecord(sl.ev_in, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(q, sl.ev_in, 0));
        }
        HIP_TRY(c, hipMemcpyAsync(cm.dev.p, cm.stage.p, t.stage_bytes, hipMemcpyHostToDevice, q));
        const uint8_t* state_in[3];
        uint8_t* sn = cm.snap.as<uint8_t>();
        for (int k = 0; k < 3; k++) {
            state_in[k] = static_cast<const uint8_t*>(t.state[k].p);
            if (!straddle || !t.state[k].bytes) continue;
            HIP_TRY(c, hipMemcpyAsync(sn, t.state[k].p, t.state[k].bytes, hipMemcpyDeviceToDevice, q));
            state_in[k] = sn;
            sn += t.state[k].bytes;
        }
        if (int rc = timed_launch(c, t.timer, [&] { return launch(cm.dev.as<uint8_t>(), state_in, rows, q); })) return rc;
        HIP_TRY(c, hipEventRecord(sl.done, q));
        HIP_TRY(c, hipEventRecord(t.owner->ev, q));
        return MIRSHA_OK;
    };
    if (t.n_seg) {
        if (int rc = queue()) return rc;  // (what it queued is drained: RingQueued)
        t.owner->queued = true;
    }
    sl.t_queued = Clock::now();
    ph[MIRSHA_PROF_PACK] = ms_since(t0);
    *n_values_out = t.values;
    ring_publish(c, sl, queued, ph, ticket_out);
    return MIRSHA_OK;
}

// ---- mirsha_streams_ring.hip: one preparation of a stream programme (n_ops > 0)
// for mirsha_streams_run and mirsha_streams_submit.  streams_prepare: every
// check, the plan into the object's scratch (`segments`: mirsha_stream_seg_plan
// into seg_stream / sfirst / seg_flags, else mirsha_stream_plan into act /
// efirst) and, host form, the packed offsets.  pack(): the entry records (16
// bytes each) to `rec` and, host form, every distinct range's bytes to
// `packed`.  window(): the aligned words the kernel reads, the device arena or
// the packed bytes at d_packed.
struct StreamPrep {
    const uint8_t* arena = nullptr;
    bool on_device = false;
    uint64_t arena_len = 0;
    uint32_t n_seg = 0, n_active = 0, entries = 0, values = 0;
    uint64_t bytes = 0;  // host form: the packed bytes
    const uint32_t* words = nullptr;
    uint32_t shift = 0, span = 0;
    void pack(mirsha_streams* st, uint8_t* rec, uint8_t* packed) const;
    void window(const uint8_t* d_packed);
};
int streams_prepare(mirsha_ctx* c, mirsha_streams* st, bool segments, const uint32_t* op_stream, const uint32_t* op_kind,
                    const uint64_t* op_off, const uint32_t* op_len, uint32_t n_ops, const uint8_t* values_out,
                    StreamPrep* p);

// ---- mirsha_plan.hip
int plan_build(mirsha_ctx* c, mirsha_pipeline* p, uint32_t n_req, const uint32_t* idx, const uint32_t* first,
               uint32_t n_lists, const uint32_t* len);
int plan_run(mirsha_ctx* c, mirsha_pipeline* p, const uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_off,
             const uint32_t* d_len, uint8_t* d_req_out, uint8_t* d_list_out);
int fused_status(mirsha_ctx* c, mirsha_pipeline* p);
void pipeline_free(mirsha_pipeline* p);
int default_pipeline_mode();

}  // namespace mirsha_api
