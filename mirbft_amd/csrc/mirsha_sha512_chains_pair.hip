// mirsha_sha512_chains_pair.hip — the producer/consumer pair route of the
// SHA-512/256 checkpoint chains:
//
//   sha512_chains_commit_pair_kernel      sha512_chains_commit_kernel's arguments
//   sha512_chains_commit_seg_pair_kernel  sha512_chains_commit_seg_kernel's arguments
//
// A chains launch has one lane per node (or per segment of a node's programme),
// so it never has more than a few 64-lane groups, and a one-lane kernel's wave
// runs its dependent compressions alone on its SIMD at what ONE wave can issue.
// Here the two waves of a 128-thread workgroup serve 64 chains: wave 0, the
// producer, does the whole walk (the entries, the row loads, the plan of each
// step, its block, the pending words and the count: none of it depends on a
// hash value, sha512_chain.h) and the message schedule with the round constants
// added; wave 1, the consumer, holds h and does nothing but the 80 rounds from
// those words, the state addition and the store of a checkpoint's row.  What
// decides bytes is sha512_chain_pair.h (proved on the CPU); this file adds the
// loaders, the ring and the barriers.
//
// Hand-over: sha512_pair_ring.h, as in mirsha_sha512_pair.hip's walked loop:
// groups of 16 rounds through two LDS slots, the producer one group ahead, one
// workgroup barrier a group; per step and lane a control word and for the group
// of 64 "another step", written by the producer before the barrier that
// precedes their reading.  __syncthreads() is the only synchronisation and
// stands outside every producer / consumer branch: both waves pass 1 + 5 *
// steps barriers, the steps counted by the LDS word.  No spinning, no atomics,
// nothing between workgroups.  The two waves touch disjoint state arrays (pend
// and cnt / h), so nothing but the ring passes between them.
//
// A translation unit and code object of its own: mirsha_sha512_chains.hip and
// every other kernel source are untouched.  The routes are at the end.
#include <hip/hip_runtime.h>

#include "../../include/mirsha.h"
#include "mirsha_chains.h"
#include "mirsha_device.h"
#include "mirsha_sha512_chains.h"
#include "mirsha_sha512_pair.h"
#include "sha512_chain_pair.h"
#include "sha512_pair_ring.h"

namespace mirsha {

static_assert(sha512::kChainCheckpoint == kCommitEntryCheckpoint, "plan entry flag");

// ---- the producer's walk -------------------------------------------------------

// A planned step and the rows it has requested (as ChainFetch,
// mirsha_sha512_chains.hip).
struct ChainPairFetch {
    sha512::ChainStep s;
    uint32_t rows[4][8];
};

// The lane's walk over ent[e .. end) from (pw, n): chain_fetch / chain_walk of
// the one-lane kernels without the compression.  Every load is guarded by the
// lane's own range [e, end): past it the index would run into the next lane's
// entries or beyond the array.  A table row is read only where the plan takes
// it; the host plan has checked every such entry against the table's size.
struct ChainPairWalk {
    const uint8_t* digests;
    const uint32_t* ent;
    uint32_t e, end;
    uint64_t n;
    uint32_t x[4];
    uint64_t pw[sha512::kChainPendWords];
    ChainPairFetch nxt;  // the step after the one handed over: planned, its rows requested

    __device__ __forceinline__ void entries() {
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = e + (uint32_t)i < end ? ent[e + (uint32_t)i] : 0u;  // e <= end <= 2^31: no wrap
    }
    __device__ __forceinline__ void fetch(ChainPairFetch& f) {
        f.s = sha512::chain_pair_plan(x, end, e, n);
#pragma unroll
        for (int sl = 0; sl < 4; sl++) {
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
            if ((f.s.take >> sl) & 1u) {
                const uint4* d = reinterpret_cast<const uint4*>(digests + 32ull * f.s.id[sl]);
                a = d[0];
                b = d[1];
            }
            f.rows[sl][0] = a.x; f.rows[sl][1] = a.y; f.rows[sl][2] = a.z; f.rows[sl][3] = a.w;
            f.rows[sl][4] = b.x; f.rows[sl][5] = b.y; f.rows[sl][6] = b.z; f.rows[sl][7] = b.w;
        }
        entries();
    }
    __device__ __forceinline__ void start(const uint8_t* digests_, const uint32_t* ent_, uint32_t e_, uint32_t end_) {
        digests = digests_;
        ent = ent_;
        e = e_;
        end = end_;
        entries();
        fetch(nxt);
    }
    // The next step: its block into w, its control word returned; the step
    // behind it is planned and its rows requested before this one's schedule.
    __device__ __forceinline__ uint32_t step(uint64_t w[16]) {
        const ChainPairFetch cur = nxt;
        fetch(nxt);
        return sha512::chain_pair_produce(pw, cur.rows, cur.s, w);
    }
};

// ---- the pair loop -------------------------------------------------------------

// The producer's part of opening step t: the lane's control word, the group's
// "another step" and, when any lane compresses, group 0 into `slot`.  A step in
// which no lane compresses (keep steps only, or every lane at its end) is the
// last call: the loop ends on its word.
__device__ __forceinline__ void open_step(ChainPairWalk& walk, Sha512PairRing& ring, uint32_t lane, uint32_t t,
                                          uint32_t slot, uint64_t w[16]) {
    const uint32_t ctl = walk.step(w);
    const bool any = __ballot(sha512::chain_pair_live(ctl)) != 0ull;
    ring.live[t & 1u][lane] = ctl;
    if (lane == 0u) ring.more[t & 1u] = any ? 1u : 0u;
    if (any) put_group<0>(w, ring.kw[slot], lane);
}

// Group G of step t: the consumer runs it from slot (t + G) & 1 (five groups a
// step, so a step's first slot alternates with the step), the producer fills
// the other slot with the group after it: G + 1 of this step, or group 0 of the
// next.  The barrier stands outside the branch.
template <int G>
__device__ __forceinline__ void chain_pair_group(ChainPairWalk& walk, Sha512PairRing& ring, bool producer, uint32_t lane,
                                                 uint32_t t, uint64_t w[16], uint64_t v[8]) {
    const uint32_t rd = (t + (uint32_t)G) & 1u, wr = rd ^ 1u;
    if (producer) {
        if constexpr (G + 1 < sha512::kPairGroups) {
            put_group<G + 1>(w, ring.kw[wr], lane);
        } else {
            open_step(walk, ring, lane, t + 1u, wr, w);
        }
    } else {
        take_group(ring.kw[rd], lane, v);
    }
    __syncthreads();
}

// The loop of both kernels.  The trip condition and a lane's control word are
// ring.more / ring.live of the step, written by the producer before the barrier
// that precedes their reading; a slot of either is rewritten two steps later,
// nine barriers after it was read.  Checkpoint rows are plain 128-bit vector
// stores (`out` may be page-locked host memory).
__device__ __forceinline__ void chain_pair_loop(ChainPairWalk& walk, Sha512PairRing& ring, bool producer, uint32_t lane,
                                                uint64_t st[8], uint4* out) {
    uint64_t w[16] = {};  // the producer's schedule window
    uint64_t v[8] = {};   // the consumer's working variables
    if (producer) open_step(walk, ring, lane, 0u, 0u, w);
    __syncthreads();
    for (uint32_t t = 0;; t++) {
        if (__builtin_amdgcn_readfirstlane((int)ring.more[t & 1u]) == 0) break;
        const uint32_t ctl = ring.live[t & 1u][lane];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = st[i];
        chain_pair_group<0>(walk, ring, producer, lane, t, w, v);
        chain_pair_group<1>(walk, ring, producer, lane, t, w, v);
        chain_pair_group<2>(walk, ring, producer, lane, t, w, v);
        chain_pair_group<3>(walk, ring, producer, lane, t, w, v);
        chain_pair_group<4>(walk, ring, producer, lane, t, w, v);
        if (!producer) {
            uint32_t d[8];
            if (sha512::chain_pair_finish(st, v, ctl, d)) {
                uint4* o = out + 2ull * sha512::chain_pair_row(ctl);
                o[0] = make_uint4(d[0], d[1], d[2], d[3]);
                o[1] = make_uint4(d[4], d[5], d[6], d[7]);
            }
        }
    }
}

// ---- kernels -------------------------------------------------------------------

// Lane k of the launch serves active chain act[k], as sha512_chains_commit_kernel.
__global__ __launch_bounds__(kSha512PairThreads) void sha512_chains_commit_pair_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ act,
    const uint32_t* __restrict__ efirst, uint32_t n_active, uint64_t* __restrict__ h, uint64_t* __restrict__ pend,
    uint64_t* __restrict__ cnt, uint4* __restrict__ out) {
    __shared__ Sha512PairRing ring;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = is_producer();
    const uint32_t k = blockIdx.x * 64u + lane;
    const bool valid = k < n_active;
    const uint32_t c = valid ? act[k] : 0u;
    uint64_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    ChainPairWalk walk;
    if (producer) {
#pragma unroll
        for (int i = 0; i < (int)sha512::kChainPendWords; i++) walk.pw[i] = valid ? pend[12ull * c + i] : 0u;
        walk.n = valid ? cnt[c] : 0u;
        walk.start(digests, ent, valid ? efirst[k] : 0u, valid ? efirst[k + 1] : 0u);
    } else if (valid) {
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = h[8ull * c + i];
    }
    chain_pair_loop(walk, ring, producer, lane, st, out);
    if (!valid) return;
    if (producer) {
#pragma unroll
        for (int i = 0; i < (int)sha512::kChainPendWords; i++) pend[12ull * c + i] = walk.pw[i];
        cnt[c] = walk.n;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) h[8ull * c + i] = st[i];
    }
}

// Lane k serves segment k of a commit ticket, as sha512_chains_commit_seg_kernel:
// a lane that is not its chain's FIRST segment starts from Hasher(), only a LAST
// one stores the state it ends in, and both waves take the issue priority once
// at entry.  FIRST lanes read h_in / pend_in / cnt_in (the chains' own arrays or
// the host's copy of them, so they are not __restrict__).  The producer reads
// and writes pend and cnt only, the consumer h only, each in its own program
// order, so a chain whose FIRST and LAST segment lie in this workgroup reads
// its state before it is overwritten, as in the one-lane kernel.
__global__ __launch_bounds__(kSha512PairThreads) void sha512_chains_commit_seg_pair_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ seg_chain,
    const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ seg_flags, uint32_t n_seg, const uint64_t* h_in,
    const uint64_t* pend_in, const uint64_t* cnt_in, uint64_t* h, uint64_t* pend, uint64_t* cnt, uint4* out,
    uint32_t prio) {
    seg_prio(prio);
    __shared__ Sha512PairRing ring;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = is_producer();
    const uint32_t k = blockIdx.x * 64u + lane;
    const bool valid = k < n_seg;
    const uint32_t c = valid ? seg_chain[k] : 0u;
    const uint32_t flags = valid ? seg_flags[k] : 0u;
    const bool first = (flags & MIRSHA_COMMIT_SEG_FIRST) != 0u, last = (flags & MIRSHA_COMMIT_SEG_LAST) != 0u;
    uint64_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    ChainPairWalk walk;
    if (producer) {
#pragma unroll
        for (int i = 0; i < (int)sha512::kChainPendWords; i++) walk.pw[i] = first ? pend_in[12ull * c + i] : 0u;
        walk.n = first ? cnt_in[c] : 0u;
        walk.start(digests, ent, valid ? sfirst[k] : 0u, valid ? sfirst[k + 1] : 0u);
    } else if (first) {
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = h_in[8ull * c + i];
    }
    chain_pair_loop(walk, ring, producer, lane, st, out);
    if (!last) return;
    if (producer) {
#pragma unroll
        for (int i = 0; i < (int)sha512::kChainPendWords; i++) pend[12ull * c + i] = walk.pw[i];
        cnt[c] = walk.n;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) h[8ull * c + i] = st[i];
    }
}

// ---- routes --------------------------------------------------------------------

namespace {

// launch_sha512_msgs' rule (mirsha_sha512_pair.h) for a launch of n lanes.
bool takes_pair(uint32_t n, int variant) {
    if (variant == kVariantPair) return true;
    if (variant == kVariantDirect || variant == kVariantLdsOnly) return false;
    return (n + 63u) / 64u <= sha512_pair_max_groups();
}

uint64_t* u64(void* p) { return static_cast<uint64_t*>(p); }
const uint64_t* u64(const void* p) { return static_cast<const uint64_t*>(p); }

}  // namespace

hipError_t launch_sha512_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                       const uint32_t* efirst, uint32_t n_active, void* h, void* pend,
                                       uint64_t* cnt, uint8_t* out, int variant, hipStream_t s,
                                       uint64_t* pair_launches) {
    if (n_active == 0 || !takes_pair(n_active, variant))
        return launch_sha512_chains_commit(digests, ent, act, efirst, n_active, h, pend, cnt, out, s);
    launch_k(sha512_chains_commit_pair_kernel, (n_active + 63u) / 64u, kSha512PairThreads, 0, s, digests, ent, act,
             efirst, n_active, u64(h), u64(pend), cnt, reinterpret_cast<uint4*>(out));
    if (pair_launches) ++*pair_launches;
    return hipGetLastError();
}

hipError_t launch_sha512_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                           const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                           const void* h_in, const void* pend_in, const uint64_t* cnt_in, void* h,
                                           void* pend, uint64_t* cnt, uint8_t* out, uint32_t prio, int variant,
                                           hipStream_t s, uint64_t* pair_launches) {
    if (n_seg == 0 || !takes_pair(n_seg, variant))
        return launch_sha512_chains_commit_seg(digests, ent, seg_chain, sfirst, seg_flags, n_seg, h_in, pend_in, cnt_in,
                                               h, pend, cnt, out, prio, s);
    launch_k(sha512_chains_commit_seg_pair_kernel, (n_seg + 63u) / 64u, kSha512PairThreads, 0, s, digests, ent,
             seg_chain, sfirst, seg_flags, n_seg, u64(h_in), u64(pend_in), cnt_in, u64(h), u64(pend), cnt,
             reinterpret_cast<uint4*>(out), prio);
    if (pair_launches) ++*pair_launches;
    return hipGetLastError();
}

}  // namespace mirsha
