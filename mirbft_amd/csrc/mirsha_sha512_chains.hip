// mirsha_sha512_chains.hip — the checkpoint chains of the second hasher,
// SHA-512/256: the device form of the testengine log's ActiveHash
// (testengine/recorder.go:186-256) when the node's Hasher is
// sha512.New512_256.  Four kernels and nothing else:
//
//   sha512_chains_commit_kernel      one lane per active chain: a cycle's
//                                    programme of writes and checkpoints
//                                    (mirsha_chains_commit; mirsha_chains_absorb
//                                    is a programme without checkpoints)
//   sha512_chains_sum_kernel         Sum() from a copy of the state
//   sha512_chains_reset_kernel       back to Hasher()
//   sha512_chains_commit_seg_kernel  one lane per segment of a commit ticket
//
// A translation unit and code object of its own, as mirsha_sha512.hip.  What
// decides bytes (the plan of a step, the block) is sha512_chain.h, proved on
// the CPU; this file adds the loaders and the walk.  No LDS, no atomics, no
// waiting; lanes depend on each other only through the walk's ballot.
#include "mirsha_sha512_chains.h"

#include <cstring>

#include "../../include/mirsha.h"
#include "mirsha_chains.h"
#include "mirsha_device.h"
#include "sha512_chain.h"

namespace mirsha {

static_assert(sha512::kChainCheckpoint == kCommitEntryCheckpoint, "plan entry flag");

// One wave a workgroup (as kStreamWave, mirsha_streams.h): these are
// latency-bound walks, one wave per 64 chains, and single-wave workgroups
// spread them over the CUs.  The compression, 12 pending words and a
// prefetched step (four entries, eight 128-bit rows) need more registers than
// the plain SHA-512/256 kernels; nothing here asks for occupancy.
constexpr uint32_t kChainWave = 64;

// A planned step and the rows it has requested.
struct ChainFetch {
    sha512::ChainStep s;
    uint32_t rows[4][8];
};

// Plans the lane's step at entry e (x[i] = ent[e + i], each loaded only below
// `end`), requests the rows of its writes, moves e and the digest count n past
// it and loads the entries of the step after it.  Every load is guarded by the
// lane's own range [e, end): past it the index would run into the next lane's
// entries or beyond the array (the notes on pos in chains_absorb_kernel and on
// commit_fetch).  A table row is read only where the plan takes it; the host
// plan has checked every such entry against the table's size.
__device__ __forceinline__ void chain_fetch(const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent,
                                            uint32_t end, uint32_t& e, uint64_t& n, uint32_t x[4], ChainFetch& f) {
    f.s = sha512::chain_plan(x, end - e, n);  // e <= end
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
    e += f.s.consumed;
    n = f.s.n_after;
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = e + (uint32_t)i < end ? ent[e + (uint32_t)i] : 0u;  // e <= end <= 2^31: no wrap
}

// The walk of a lane over entries ent[e .. end) from the state (st, pw, n).
// Wave-uniform: a lane whose step does nothing has reached its end (only a
// programme's last step can be without a compression).  The step after this
// one is planned and its rows requested before this step's 80 rounds.
// Checkpoint rows are plain 128-bit vector stores (`out` may be page-locked
// host memory).
__device__ __forceinline__ void chain_walk(const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent,
                                           uint32_t e, uint32_t end, uint64_t st[8],
                                           uint64_t pw[sha512::kChainPendWords], uint64_t& n, uint4* out) {
    uint32_t x[4];
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = e + (uint32_t)i < end ? ent[e + (uint32_t)i] : 0u;
    ChainFetch cur;
    chain_fetch(digests, ent, end, e, n, x, cur);
    while (__ballot(cur.s.full || cur.s.cp || cur.s.keep) != 0ull) {
        ChainFetch nxt;
        chain_fetch(digests, ent, end, e, n, x, nxt);
        uint64_t w[16];
        sha512::chain_block(pw, cur.rows, cur.s, w);
        if (cur.s.keep) sha512::chain_keep(w, pw);
        if (cur.s.full || cur.s.cp) sha512::compress(st, w);
        if (cur.s.cp) {
            uint32_t d[8];
            sha512::digest_words(st, d);
            uint4* o = out + 2ull * cur.s.row;
            o[0] = make_uint4(d[0], d[1], d[2], d[3]);
            o[1] = make_uint4(d[4], d[5], d[6], d[7]);
#pragma unroll
            for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
        }
        cur = nxt;
    }
}

__device__ __forceinline__ void chain_state_load(const uint64_t* h, const uint64_t* pend, const uint64_t* cnt,
                                                 uint32_t c, uint64_t st[8], uint64_t pw[sha512::kChainPendWords],
                                                 uint64_t& n) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = h[8ull * c + i];
#pragma unroll
    for (int i = 0; i < (int)sha512::kChainPendWords; i++) pw[i] = pend[12ull * c + i];
    n = cnt[c];
}

__device__ __forceinline__ void chain_state_store(uint64_t* h, uint64_t* pend, uint64_t* cnt, uint32_t c,
                                                  const uint64_t st[8], const uint64_t pw[sha512::kChainPendWords],
                                                  uint64_t n) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[8ull * c + i] = st[i];
#pragma unroll
    for (int i = 0; i < (int)sha512::kChainPendWords; i++) pend[12ull * c + i] = pw[i];
    cnt[c] = n;
}

// One lane per chain that has entries this call (mirsha_commit_plan): entries
// ent[efirst[k] .. efirst[k+1]) in op order, null writes already removed.  The
// state left behind is the same whichever call wrote it, so the calls mix
// freely on one mirsha_chains.
__global__ __launch_bounds__(kChainWave) void sha512_chains_commit_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ act,
    const uint32_t* __restrict__ efirst, uint32_t n_active, uint64_t* __restrict__ h, uint64_t* __restrict__ pend,
    uint64_t* __restrict__ cnt, uint4* __restrict__ out) {
    const uint32_t k = blockIdx.x * kChainWave + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t c = valid ? act[k] : 0u;
    const uint32_t e = valid ? efirst[k] : 0u;
    const uint32_t end = valid ? efirst[k + 1] : 0u;
    uint64_t st[8], pw[sha512::kChainPendWords];
    uint64_t n = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
#pragma unroll
    for (int i = 0; i < (int)sha512::kChainPendWords; i++) pw[i] = 0u;
    if (valid) chain_state_load(h, pend, cnt, c, st, pw, n);
    chain_walk(digests, ent, e, end, st, pw, n, out);
    if (valid) chain_state_store(h, pend, cnt, c, st, pw, n);
}

// Sum(nil) of chains which[0..k): the final block (the pending rows, 0x80, the
// bit length) from a copy of the state.
__global__ __launch_bounds__(kChainWave) void sha512_chains_sum_kernel(const uint32_t* __restrict__ which, uint32_t k_n,
                                                                       const uint64_t* __restrict__ h,
                                                                       const uint64_t* __restrict__ pend,
                                                                       const uint64_t* __restrict__ cnt,
                                                                       uint4* __restrict__ out) {
    const uint32_t k = blockIdx.x * kChainWave + threadIdx.x;
    if (k >= k_n) return;
    const uint32_t c = which[k];
    uint64_t st[8], pw[sha512::kChainPendWords], w[16];
    uint64_t n;
    chain_state_load(h, pend, cnt, c, st, pw, n);
    uint32_t rows[4][8];
#pragma unroll
    for (int sl = 0; sl < 4; sl++)
#pragma unroll
        for (int i = 0; i < 8; i++) rows[sl][i] = 0u;
    sha512::chain_block(pw, rows, sha512::chain_sum_step(n), w);
    sha512::compress(st, w);
    uint32_t d[8];
    sha512::digest_words(st, d);
    out[2ull * k] = make_uint4(d[0], d[1], d[2], d[3]);
    out[2ull * k + 1u] = make_uint4(d[4], d[5], d[6], d[7]);
}

__global__ __launch_bounds__(kChainWave) void sha512_chains_reset_kernel(const uint32_t* __restrict__ which,
                                                                         uint32_t k_n, uint64_t* __restrict__ h,
                                                                         uint64_t* __restrict__ cnt) {
    const uint32_t k = blockIdx.x * kChainWave + threadIdx.x;
    if (k >= k_n) return;
    const uint32_t c = which[k];
#pragma unroll
    for (int i = 0; i < 8; i++) h[8ull * c + i] = sha512::kH0[i];
    cnt[c] = 0u;
}

// One lane per segment of a cycle's commit programme (mirsha_commit_seg_plan),
// as chains_commit_seg_kernel (mirsha_chains.hip): a lane that is not its
// chain's FIRST segment starts from Hasher(), only a LAST one stores the state
// it ends in, and the wave takes its issue priority once at entry.  FIRST lanes
// read h_in / pend_in / cnt_in: the chains' own arrays, or the copy of them the
// host took ahead of the launch when a chain's FIRST and LAST segment lie in
// different waves (so they are not __restrict__).
__global__ __launch_bounds__(kChainWave) void sha512_chains_commit_seg_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ seg_chain,
    const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ seg_flags, uint32_t n_seg, const uint64_t* h_in,
    const uint64_t* pend_in, const uint64_t* cnt_in, uint64_t* h, uint64_t* pend, uint64_t* cnt, uint4* out,
    uint32_t prio) {
    seg_prio(prio);
    const uint32_t k = blockIdx.x * kChainWave + threadIdx.x;
    const bool valid = k < n_seg;
    const uint32_t c = valid ? seg_chain[k] : 0u;
    const uint32_t flags = valid ? seg_flags[k] : 0u;
    const uint32_t e = valid ? sfirst[k] : 0u;
    const uint32_t end = valid ? sfirst[k + 1] : 0u;
    uint64_t st[8], pw[sha512::kChainPendWords];
    uint64_t n = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
#pragma unroll
    for (int i = 0; i < (int)sha512::kChainPendWords; i++) pw[i] = 0u;
    if (flags & MIRSHA_COMMIT_SEG_FIRST) chain_state_load(h_in, pend_in, cnt_in, c, st, pw, n);
    chain_walk(digests, ent, e, end, st, pw, n, out);
    if (flags & MIRSHA_COMMIT_SEG_LAST) chain_state_store(h, pend, cnt, c, st, pw, n);
}

void sha512_chains_h0(void* h) { memcpy(h, sha512::kH0, sizeof(sha512::kH0)); }

namespace {
uint64_t* u64(void* p) { return static_cast<uint64_t*>(p); }
const uint64_t* u64(const void* p) { return static_cast<const uint64_t*>(p); }
}  // namespace

hipError_t launch_sha512_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                       const uint32_t* efirst, uint32_t n_active, void* h, void* pend,
                                       uint64_t* cnt, uint8_t* out, hipStream_t s) {
    if (n_active == 0) return hipSuccess;
    launch_k(sha512_chains_commit_kernel, (n_active + kChainWave - 1u) / kChainWave, kChainWave, 0, s, digests, ent, act,
             efirst, n_active, u64(h), u64(pend), cnt, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_sha512_chains_sum(const uint32_t* which, uint32_t k, const void* h, const void* pend,
                                    const uint64_t* cnt, uint8_t* out, hipStream_t s) {
    if (k == 0) return hipSuccess;
    launch_k(sha512_chains_sum_kernel, (k + kChainWave - 1u) / kChainWave, kChainWave, 0, s, which, k, u64(h), u64(pend),
             cnt, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_sha512_chains_reset(const uint32_t* which, uint32_t k, void* h, uint64_t* cnt, hipStream_t s) {
    if (k == 0) return hipSuccess;
    launch_k(sha512_chains_reset_kernel, (k + kChainWave - 1u) / kChainWave, kChainWave, 0, s, which, k, u64(h), cnt);
    return hipGetLastError();
}

hipError_t launch_sha512_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                           const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                           const void* h_in, const void* pend_in, const uint64_t* cnt_in, void* h,
                                           void* pend, uint64_t* cnt, uint8_t* out, uint32_t prio, hipStream_t s) {
    if (n_seg == 0) return hipSuccess;
    launch_k(sha512_chains_commit_seg_kernel, (n_seg + kChainWave - 1u) / kChainWave, kChainWave, 0, s, digests, ent,
             seg_chain, sfirst, seg_flags, n_seg, u64(h_in), u64(pend_in), cnt_in, u64(h), u64(pend), cnt,
             reinterpret_cast<uint4*>(out), prio);
    return hipGetLastError();
}

}  // namespace mirsha
