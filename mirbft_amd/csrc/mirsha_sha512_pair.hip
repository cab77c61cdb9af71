// mirsha_sha512_pair.hip — the producer/consumer pair route of the second
// hasher, SHA-512/256, for small launches:
//
//   sha512_msgs_pair_kernel                 sha512_msgs_kernel's arguments
//   sha512_lists_pair_kernel                sha512_lists_kernel's arguments
//   sha512_plan_lists_pair_kernel<kUniform> sha512_plan_lists_kernel's arguments
//
// When a launch has fewer 64-lane groups than half the chip's SIMDs, a one-lane
// kernel's wave runs alone on its SIMD and its time is one dependent chain of
// compressions at what ONE wave can issue.  A pair splits a compression over
// the two waves of a 128-thread workgroup (two SIMDs): wave 0, the producer,
// loads the blocks and computes the message schedule with the round constants
// added, which never depends on the chaining state; wave 1, the consumer, runs
// the 80 rounds from those words.  The split itself is sha512_pair.h (proved on
// the CPU); the loaders are sha512_lanes.h, as in the one-lane kernels.
//
// Hand-over: groups of 16 rounds through a ring of two LDS slots
// (sha512_pair_ring.h, shared with the chains' pair kernels), the producer one
// group ahead, one workgroup barrier a group.  __syncthreads() is the only
// synchronisation: no spinning, no atomics, nothing between workgroups.  Both
// waves execute the same number of barriers on every input: every barrier
// stands outside the producer / consumer branch, and the block loop's trip
// count is either computed by both waves from the same lengths (messages, plan
// lists) or one LDS word that the producer writes before a barrier and both
// waves read after it (lists with nulls, whose block count only the walk
// knows).
//
// A translation unit and code object of its own: the one-lane kernels' units
// and the SHA-256 kernels' sources are untouched.  The routes (which launch
// takes a pair) are at the end of the file.
#include "mirsha_sha512_pair.h"

#include <stdlib.h>

#include "mirsha_sha512.h"
#include "mirsha_sha512_plan.h"
#include "sha512_lanes.h"
#include "sha512_pair.h"
#include "sha512_pair_ring.h"

namespace mirsha {

// ---- producer-side sources of block words ----------------------------------
// block(blk, w) is called for blocks 0, 1, 2, ... in order and returns whether
// the lane has that block; each source keeps the next block's loads in flight.

// A message of an arena at any byte alignment: sha512_msg_lane's loads.
struct Sha512MsgBlocks {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t records, o, L, nb, sel;
    RawBlock raw;
    __device__ __forceinline__ void start(const uint8_t* arena, uint64_t arena_len, uint32_t o_, uint32_t L_,
                                          uint32_t nb_) {
        records = (uint32_t)((arena_len + 3u) & ~3ull);
        rsrc = buffer_rsrc(arena, records);
        o = o_;
        L = L_;
        nb = nb_;
        sel = be_sel(o & 3u);
        issue_block(rsrc, records, o, 0u < nb, raw);
    }
    __device__ __forceinline__ bool block(uint32_t blk, uint64_t w[16]) {
        uint32_t bw[32];
#pragma unroll
        for (int k = 0; k < 32; k++) bw[k] = be_word(raw.v[k + 1], raw.v[k], sel);
        issue_block(rsrc, records, o + 128u * (blk + 1u), blk + 1u < nb, raw);  // before this block's schedule
        const uint32_t p = 128u * blk;
        if (blk < nb && (uint64_t)p + 128u > L) sha512::pad_block(bw, p, L, blk + 1u == nb);
        sha512::join_words(bw, w);
        return blk < nb;
    }
};

// A digest list with MIRSHA_NULL_INDEX entries skipped in the walk:
// sha512_list_lane's walk.  Only this wave knows how many blocks a list has.
struct Sha512ListWalk {
    __amdgpu_buffer_rsrc_t drs, irs;
    uint32_t e, e1, d0;
    ListRows cur;
    bool more;
    __device__ __forceinline__ void start(__amdgpu_buffer_rsrc_t drs_, __amdgpu_buffer_rsrc_t irs_, uint32_t e0,
                                          uint32_t e1_, bool valid) {
        drs = drs_;
        irs = irs_;
        e = e0;
        e1 = e1_;
        d0 = 0u;
        more = valid;
        fetch_rows(drs, irs, e, e1, valid, cur);
    }
    __device__ __forceinline__ bool block(uint32_t /*blk*/, uint64_t w[16]) {
        const bool has = more;
        const bool last = cur.filled < 4u;
        ListRows nxt;
        fetch_rows(drs, irs, e, e1, more && !last, nxt);
        sha512::list_block(cur.rows, d0, d0 + cur.filled, last, w);
        more = more && !last;
        cur = nxt;
        d0 += 4u;
        return has;
    }
};

// A compacted list of a plan: sha512_plan_list_lane's loads.
template <bool kUniform>
struct Sha512PlanBlocks {
    __amdgpu_buffer_rsrc_t drs, irs;
    uint32_t e0, c, nb;
    uint32_t cur[4][8];
    __device__ __forceinline__ void start(__amdgpu_buffer_rsrc_t drs_, __amdgpu_buffer_rsrc_t irs_, uint32_t e0_,
                                          uint32_t c_, uint32_t nb_) {
        drs = drs_;
        irs = irs_;
        e0 = e0_;
        c = c_;
        nb = nb_;
        plan_rows<kUniform>(drs, irs, e0, c, 0u, 0u < nb, cur);
    }
    __device__ __forceinline__ bool block(uint32_t blk, uint64_t w[16]) {
        uint32_t nxt[4][8];
        plan_rows<kUniform>(drs, irs, e0, c, blk + 1u, blk + 1u < nb, nxt);
        sha512::list_block(cur, 4u * blk, c, blk + 1u == nb, w);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int i = 0; i < 8; i++) cur[s][i] = nxt[s][i];
        return blk < nb;
    }
};

// ---- the pair loop -----------------------------------------------------------

// The producer's part of opening block `blk`: its words, the walked loop's
// flags, and group 0 into `slot` when any lane of the group has the block.
// kWalked: always called (the walk decides); counted: only when the block is
// within the trip count.
template <bool kWalked, class Src>
__device__ __forceinline__ void open_block(Src& src, Sha512PairRing& ring, uint32_t lane, uint32_t blk, uint32_t slot,
                                           uint64_t w[16]) {
    const bool has = src.block(blk, w);
    bool any = true;
    if (kWalked) {
        any = __ballot(has) != 0ull;
        ring.live[blk & 1u][lane] = has ? 1u : 0u;
        if (lane == 0u) ring.more[blk & 1u] = any ? 1u : 0u;
    }
    if (any) put_group<0>(w, ring.kw[slot], lane);
}

// Step G of block blk: the consumer runs group G from slot (blk + G) & 1 (five
// groups a block, so a block's first slot alternates with the block), the
// producer fills the other slot with the group after it: G + 1 of this block,
// or group 0 of the next.  The barrier stands outside the branch.
template <int G, bool kWalked, class Src>
__device__ __forceinline__ void pair_step(Src& src, Sha512PairRing& ring, bool producer, uint32_t lane, uint32_t blk,
                                          bool next_block, uint64_t w[16], uint64_t v[8]) {
    const uint32_t rd = (blk + (uint32_t)G) & 1u, wr = rd ^ 1u;
    if (producer) {
        if constexpr (G + 1 < sha512::kPairGroups) {
            put_group<G + 1>(w, ring.kw[wr], lane);
        } else {
            if (kWalked || next_block) open_block<kWalked>(src, ring, lane, blk + 1u, wr, w);
        }
    } else {
        take_group(ring.kw[rd], lane, v);
    }
    __syncthreads();
}

// The loop shared by the three kernels.  Counted (!kWalked): both waves hold
// the same nb per lane (they serve the same 64 messages), so wave_max(nb) is
// the same trip count in both.  kWalked: the trip condition and a lane's
// liveness are ring.more / ring.live of the block, written by the producer
// before the barrier that precedes their reading; nb is not used.  A slot of
// either is rewritten two blocks later, ten barriers after it was read.
template <bool kWalked, class Src>
__device__ __forceinline__ void sha512_pair_loop(Src& src, Sha512PairRing& ring, bool producer, uint32_t lane,
                                                 uint32_t nb, uint64_t st[8]) {
    const uint32_t wave_nb = kWalked ? 0u : wave_max(nb);
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    uint64_t w[16] = {};  // the producer's schedule window
    uint64_t v[8] = {};   // the consumer's working variables
    if (producer && (kWalked || wave_nb != 0u)) open_block<kWalked>(src, ring, lane, 0u, 0u, w);
    __syncthreads();
    for (uint32_t blk = 0;; blk++) {
        bool live;
        if (kWalked) {
            if (__builtin_amdgcn_readfirstlane((int)ring.more[blk & 1u]) == 0) break;
            live = ring.live[blk & 1u][lane] != 0u;
        } else {
            if (blk >= wave_nb) break;
            live = blk < nb;
        }
        const bool next_block = blk + 1u < wave_nb;
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = st[i];
        pair_step<0, kWalked>(src, ring, producer, lane, blk, next_block, w, v);
        pair_step<1, kWalked>(src, ring, producer, lane, blk, next_block, w, v);
        pair_step<2, kWalked>(src, ring, producer, lane, blk, next_block, w, v);
        pair_step<3, kWalked>(src, ring, producer, lane, blk, next_block, w, v);
        pair_step<4, kWalked>(src, ring, producer, lane, blk, next_block, w, v);
        if (!producer) sha512::finish_block(st, v, live);
    }
}

// ---- kernels -----------------------------------------------------------------

// Lane `slot` of the launch hashes message order[slot] (order == NULL:
// identity), as sha512_msgs_kernel.
__global__ __launch_bounds__(kSha512PairThreads) void sha512_msgs_pair_kernel(
    const uint8_t* __restrict__ arena, uint64_t arena_len, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, const uint32_t* __restrict__ order, uint32_t n, uint8_t* __restrict__ out) {
    __shared__ Sha512PairRing ring;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = is_producer();
    const uint32_t slot = blockIdx.x * 64u + lane;
    const bool valid = slot < n;
    const uint32_t msg = valid ? (order ? order[slot] : slot) : 0u;
    const uint32_t L = valid ? len[msg] : 0u;
    const uint32_t nb = valid ? sha512::blocks_for_len(L) : 0u;
    Sha512MsgBlocks src;
    if (producer) src.start(arena, arena_len, valid ? (uint32_t)off[msg] : 0u, L, nb);
    uint64_t st[8];
    sha512_pair_loop<false>(src, ring, producer, lane, nb, st);
    if (!producer && valid) store_sha512_digest(out, msg, st);
}

// Lane k hashes list k, nulls skipped in the walk, as sha512_lists_kernel.
__global__ __launch_bounds__(kSha512PairThreads) void sha512_lists_pair_kernel(
    const uint8_t* __restrict__ digests, uint32_t n_digests, const uint32_t* __restrict__ idx, uint32_t n_entries,
    const uint32_t* __restrict__ first, uint32_t n_lists, uint8_t* __restrict__ out) {
    __shared__ Sha512PairRing ring;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = is_producer();
    const uint32_t k = blockIdx.x * 64u + lane;
    const bool valid = k < n_lists;
    Sha512ListWalk src;
    if (producer)
        src.start(buffer_rsrc(digests, 32u * n_digests), buffer_rsrc(idx, 4u * n_entries), valid ? first[k] : 0u,
                  valid ? first[k + 1] : 0u, valid);
    uint64_t st[8];
    sha512_pair_loop<true>(src, ring, producer, lane, 0u, st);
    if (!producer && valid) store_sha512_digest(out, k, st);
}

// Lane k hashes compacted list k of a plan, as sha512_plan_lists_kernel
// (kUniform, `uniform`: identity lists of B entries, sha512_plan_list_lane).
template <bool kUniform>
__global__ __launch_bounds__(kSha512PairThreads) void sha512_plan_lists_pair_kernel(
    const uint8_t* __restrict__ digests, uint32_t n_digests, const uint32_t* __restrict__ cidx, uint32_t n_entries,
    const uint32_t* __restrict__ cfirst, uint32_t n_lists, uint32_t uniform, uint8_t* __restrict__ out) {
    __shared__ Sha512PairRing ring;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = is_producer();
    const uint32_t k = blockIdx.x * 64u + lane;
    const bool valid = k < n_lists;
    uint32_t e0 = 0u, c = 0u;
    if (valid) {
        if (kUniform) {
            e0 = k * uniform;  // (k B < n_entries: uniform_lists)
            c = min(uniform, n_entries - e0);
        } else {
            e0 = cfirst[k];
            c = cfirst[k + 1] - e0;
        }
    }
    const uint32_t nb = valid ? c / 4u + 1u : 0u;
    Sha512PlanBlocks<kUniform> src;
    if (producer) src.start(buffer_rsrc(digests, 32u * n_digests), buffer_rsrc(cidx, 4u * n_entries), e0, c, nb);
    uint64_t st[8];
    sha512_pair_loop<false>(src, ring, producer, lane, nb, st);
    if (!producer && valid) store_sha512_digest(out, k, st);
}

// ---- routes ------------------------------------------------------------------

uint32_t sha512_pair_max_groups() {
    static const uint32_t v = [] {
        const char* e = ab_getenv("MIRSHA_SHA512_PAIR");
        if (e && e[0] == '0') return 0u;
        const char* m = ab_getenv("MIRSHA_SHA512_PAIR_MAX_GROUPS");
        return m ? (uint32_t)strtoul(m, nullptr, 10) : kSha512PairMaxGroups;
    }();
    return v;
}

static bool few_groups(uint32_t n) { return (n + 63u) / 64u <= sha512_pair_max_groups(); }
static void count_pair(uint64_t* pair_launches) {
    if (pair_launches) ++*pair_launches;
}

hipError_t launch_sha512_msgs(const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                              const uint32_t* order, uint32_t n, uint8_t* out, int variant, hipStream_t s,
                              uint64_t* pair_launches) {
    const bool one_lane = variant == kVariantDirect || variant == kVariantLdsOnly;
    if (n == 0 || one_lane || !(variant == kVariantPair || few_groups(n)))
        return launch_sha512_msgs(arena, arena_len, off, len, order, n, out, s);
    if (arena_len > kMaxBufferArena || n >= kMaxBufferMsgs) return hipErrorInvalidValue;
    launch_k(sha512_msgs_pair_kernel, (n + 63u) / 64u, kSha512PairThreads, 0, s, arena, arena_len, off, len, order, n,
             out);
    count_pair(pair_launches);
    return hipGetLastError();
}

hipError_t launch_sha512_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* idx, uint32_t n_entries,
                               const uint32_t* first, uint32_t n_lists, uint32_t* scratch, uint8_t* out, hipStream_t s,
                               uint64_t* pair_launches) {
    if (n_lists == 0 || !few_groups(n_lists))
        return launch_sha512_lists(digests, n_digests, idx, n_entries, first, n_lists, scratch, out, s);
    launch_k(sha512_lists_pair_kernel, (n_lists + 63u) / 64u, kSha512PairThreads, 0, s, digests, n_digests, idx,
             n_entries, first, n_lists, out);
    count_pair(pair_launches);
    return hipGetLastError();
}

hipError_t launch_sha512_plan_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* cidx,
                                    uint32_t n_entries, const uint32_t* cfirst, uint32_t n_lists, uint32_t uniform,
                                    uint8_t* out, hipStream_t s, uint64_t* pair_launches) {
    if (n_lists == 0 || !few_groups(n_lists))
        return launch_sha512_plan_lists(digests, n_digests, cidx, n_entries, cfirst, n_lists, uniform, out, s);
    const uint32_t grid = (n_lists + 63u) / 64u;
    if (uniform)
        launch_k(sha512_plan_lists_pair_kernel<true>, grid, kSha512PairThreads, 0, s, digests, n_digests, cidx,
                 n_entries, cfirst, n_lists, uniform, out);
    else
        launch_k(sha512_plan_lists_pair_kernel<false>, grid, kSha512PairThreads, 0, s, digests, n_digests, cidx,
                 n_entries, cfirst, n_lists, 0u, out);
    count_pair(pair_launches);
    return hipGetLastError();
}

}  // namespace mirsha
