// mirsha_chains.hip — streaming checkpoint chains (testengine
// NodeState.ActiveHash): the SHA-256 kernels and every mirsha_chains_* entry
// point of include/mirsha.h, the synchronous calls and the commit tickets of
// the asynchronous ring (mirsha_chains_commit_submit*: the commit stage of
// ProcessorWorkPool, commitInParallel, processor.go:363-394, :447-470, beside
// its hash stage, mirsha_async.hip).  Five kernels and nothing else:
//
//   chains_absorb_kernel      one lane per chain with new digests
//   chains_sum_kernel         Sum() from a copy of the state
//   chains_reset_kernel       back to Hasher()
//   chains_commit_kernel      one lane per active chain: a cycle's programme
//                             of writes and checkpoints
//   chains_commit_seg_kernel  one lane per segment of a commit ticket
//
// A translation unit and code object of its own: the hashing kernels keep
// theirs (mirsha_kernels.hip).  The SHA-512/256 kernels are
// mirsha_sha512_chains.hip; which set a mirsha_chains runs is one row of
// chain_kernels (mirsha_chains.h).
#include "mirsha_chains.h"

#include "mirsha_ctx.h"
#include "mirsha_sha512_chains.h"

namespace mirsha {

// Running SHA-256 states, one per application node: the checkpoint value of
// testengine/recorder.go:213-256 is Sum() of a hash that every committed
// request digest is written into (ActiveHash.Write, :223), reset at each
// checkpoint (Set, :187).  State per chain: midstate h[8], the pending
// digest of an odd count (its 8 big-endian words) and the digest count.
// Writes are 32-byte digests, so a block is always two whole digests.
__device__ __forceinline__ void load_digest_words(const uint8_t* __restrict__ digests, uint32_t p, bool live,
                                                  uint32_t w[8]) {
    if (live) {
        const uint4* d = reinterpret_cast<const uint4*>(digests + 32ull * p);
        const uint4 a = d[0], b = d[1];
        be_words(a, w);
        be_words(b, w + 4);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0u;
    }
}

__device__ __forceinline__ void chain_state_load(const uint32_t* h, const uint32_t* pend, const uint64_t* cnt,
                                                 uint32_t c, uint32_t st[8], uint32_t pw[8], uint64_t& n) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[i] = h[8ull * c + i];
        pw[i] = pend[8ull * c + i];
    }
    n = cnt[c];
}

__device__ __forceinline__ void chain_state_store(uint32_t* h, uint32_t* pend, uint64_t* cnt, uint32_t c,
                                                  const uint32_t st[8], const uint32_t pw[8], uint64_t n) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h[8ull * c + i] = st[i];
        pend[8ull * c + i] = pw[i];
    }
    cnt[c] = n;
}

// One lane per chain with new digests pos[afirst[k] .. afirst[k+1]) (in write
// order).  With `odd` = a digest pending from earlier writes, the lane
// completes (odd + m) / 2 blocks: block t = digest q ‖ digest q+1 with
// q = 2t - odd (q = -1: the pending digest).
__global__ __launch_bounds__(kBlockThreads) void chains_absorb_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ act,
    const uint32_t* __restrict__ afirst, uint32_t n_active, uint32_t* __restrict__ h, uint32_t* __restrict__ pend,
    uint64_t* __restrict__ cnt) {
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t c = valid ? act[k] : 0u;
    const uint32_t e0 = valid ? afirst[k] : 0u;
    const uint32_t m = valid ? afirst[k + 1] - e0 : 0u;
    uint32_t st[8], pw[8];
    uint64_t n = 0;
    if (valid) chain_state_load(h, pend, cnt, c, st, pw, n);
    const uint32_t odd = (uint32_t)(n & 1u);
    const uint32_t blocks = (odd + m) / 2u;
    const uint32_t steps = wave_max(blocks);
    for (uint32_t t = 0; t < steps; t++) {
        const bool live = t < blocks;
        const int32_t q = (int32_t)(2u * t) - (int32_t)odd;
        uint32_t w[16];
        if (q < 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = pw[i];
        } else {
            // Guarded like the second load below: past this lane's own block
            // count the index would run beyond its range in pos.
            load_digest_words(digests, live ? pos[e0 + (uint32_t)q] : 0u, live, w);
        }
        load_digest_words(digests, live ? pos[e0 + (uint32_t)(q + 1)] : 0u, live, w + 8);
        if (live) compress_asm_lat(st, w);
    }
    if (valid) {
        if ((odd + m) & 1u) {
            if (m) load_digest_words(digests, pos[e0 + m - 1u], true, pw);  // else the old pending stays
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            h[8ull * c + i] = st[i];
            pend[8ull * c + i] = pw[i];
        }
        cnt[c] = n + m;  // (summed behind the stores, so not chain_state_store: the schedule is kept)
    }
}

// Sum(nil) of chains which[0..k): the final padded block (pending digest, if
// any, then 0x80 and the 64-bit bit length) from a copy of the midstate.  (Its
// loads are per-word conditional, not chain_state_load's.)
__global__ __launch_bounds__(kBlockThreads) void chains_sum_kernel(const uint32_t* __restrict__ which, uint32_t k_n,
                                                                   const uint32_t* __restrict__ h,
                                                                   const uint32_t* __restrict__ pend,
                                                                   const uint64_t* __restrict__ cnt,
                                                                   uint8_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool valid = k < k_n;
    const uint32_t c = valid ? which[k] : 0u;
    uint32_t st[8], w[16];
    const uint64_t n = valid ? cnt[c] : 0u;
    const bool odd = (n & 1u) != 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[i] = valid ? h[8ull * c + i] : 0u;
        w[i] = odd ? pend[8ull * c + i] : 0u;
        w[8 + i] = 0u;
    }
    w[odd ? 8 : 0] = 0x80000000u;
    const uint64_t bits = n * 256u;
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    compress_asm_lat(st, w);
    if (valid) store_digest(out, k, st);
}

__global__ __launch_bounds__(kBlockThreads) void chains_reset_kernel(const uint32_t* __restrict__ which, uint32_t k_n,
                                                                     uint32_t* __restrict__ h,
                                                                     uint64_t* __restrict__ cnt) {
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    if (k >= k_n) return;
    const uint32_t c = which[k];
#pragma unroll
    for (int i = 0; i < 8; i++) h[8ull * c + i] = kH0[i];
    cnt[c] = 0u;
}

// ---- one step of a commit programme ---------------------------------------
// A step is at most one compression: two whole digests (the first may be the
// digest pending from earlier writes), or the final padded block of a
// checkpoint (pending digest, if any, 0x80, bit length: always one block), or
// a lone last write that becomes the pending digest without a compression.
struct CommitStep {
    uint4 a0, a1, b0, b1;  // raw rows of the two halves (zeros where the step loads none)
    uint64_t bits;         // checkpoint: the message's bit length
    uint32_t row;          // checkpoint: output row
    bool use_pend;         // first half = the pending digest
    bool have_a;           // checkpoint: a first half precedes the 0x80
    bool write, cp;        // compress two digests / the final block (neither: nothing to hash)
    bool keep;             // a lone last write: the first half becomes the pending digest
};

// Plans step t of a lane at entry e (x0 = ent[e], xn = ent[e + 1], each
// loaded only below `end`), requests its digest rows, moves e and the digest
// count n past it and loads the entries of step t + 1.  Which entries a step
// consumes depends on the entry kinds and the parity only, never on a hash
// value, so this walk runs one step ahead of the hashing.  Every load is
// guarded by the lane's own range: past `end` the index would run into the
// next lane's entries or beyond the array (the note on pos in
// chains_absorb_kernel).
__device__ __forceinline__ CommitStep commit_fetch(const uint8_t* __restrict__ digests,
                                                   const uint32_t* __restrict__ ent, uint32_t end, uint32_t& e,
                                                   uint64_t& n, uint32_t& x0, uint32_t& xn) {
    CommitStep s;
    const bool live = e < end;
    const bool odd = (n & 1u) != 0u;
    const bool take0 = live && !odd && !(x0 & kCommitEntryCheckpoint);  // first half from the table
    const uint32_t e1 = e + (take0 ? 1u : 0u);
    const bool live1 = live && e1 < end;  // odd && live: e1 == e, so live1
    const uint32_t x1 = take0 ? xn : x0;
    s.write = live1 && !(x1 & kCommitEntryCheckpoint);
    s.cp = live1 && (x1 & kCommitEntryCheckpoint) != 0u;
    s.use_pend = odd && live1;
    s.have_a = odd || take0;
    s.keep = take0 && !live1;
    s.row = x1 & ~kCommitEntryCheckpoint;
    s.bits = (n + (take0 ? 1u : 0u)) * 256u;
    s.a0 = s.a1 = s.b0 = s.b1 = make_uint4(0u, 0u, 0u, 0u);
    if (take0) {
        const uint4* d = reinterpret_cast<const uint4*>(digests + 32ull * x0);
        s.a0 = d[0];
        s.a1 = d[1];
    }
    if (s.write) {
        const uint4* d = reinterpret_cast<const uint4*>(digests + 32ull * x1);
        s.b0 = d[0];
        s.b1 = d[1];
    }
    n = s.cp ? 0u : n + (take0 ? 1u : 0u) + (s.write ? 1u : 0u);
    e = e1 + (live1 ? 1u : 0u);
    x0 = e < end ? ent[e] : 0u;
    xn = e + 1u < end ? ent[e + 1u] : 0u;  // e <= end <= 2^31: no wrap
    return s;
}

// The walk of a lane over entries ent[e .. end) from the state (st, pw, n).
// After a checkpoint the lane's state is Hasher() again.  The walk runs one
// step ahead of the hashing: the next step's entries were loaded a step
// earlier, its digest rows are requested before this step's compression and
// first touched (byte swap) after it.  A lone lane then pays max(compression,
// one load) per step, not their sum.  Checkpoint rows are plain 128-bit vector
// stores (`out` may be host-visible page-locked memory).
__device__ __forceinline__ void commit_walk(const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent,
                                            uint32_t& e, uint32_t end, uint32_t st[8], uint32_t pw[8], uint64_t& n,
                                            uint8_t* out) {
    uint32_t x0 = e < end ? ent[e] : 0u;
    uint32_t xn = e + 1u < end ? ent[e + 1u] : 0u;
    CommitStep s = commit_fetch(digests, ent, end, e, n, x0, xn);
    // Wave-uniform: a lane whose step does nothing has reached its end (only a
    // programme's last step can be without a compression).
    while (__ballot(s.write || s.cp || s.keep) != 0ull) {
        const CommitStep nx = commit_fetch(digests, ent, end, e, n, x0, xn);
        uint32_t w[16];
        be_words(s.a0, w); be_words(s.a1, w + 4); be_words(s.b0, w + 8); be_words(s.b1, w + 12);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (s.use_pend) w[i] = pw[i];
            if (s.keep) pw[i] = w[i];
        }
        if (s.cp) {
            if (s.have_a) w[8] = 0x80000000u; else w[0] = 0x80000000u;
            w[14] = (uint32_t)(s.bits >> 32);
            w[15] = (uint32_t)s.bits;
        }
        if (s.write || s.cp) compress_asm_lat(st, w);
        if (s.cp) {
            store_digest(out, s.row, st);
#pragma unroll
            for (int i = 0; i < 8; i++) st[i] = kH0[i];
        }
        s = nx;
    }
}

// ---- a cycle's Commits in one launch (processor.go:145-168) -----------------
// The commit loop of Processor.Process applies every committed batch to the
// application log and takes the log's value at each checkpoint; with the
// testengine's log (NodeState.Commit, testengine/recorder.go:213-256) that is
// a programme of Write(digest) and Sum-then-fresh-hasher per node.  One lane
// per chain that has entries this cycle (mirsha_commit_plan): entries
// ent[efirst[k] .. efirst[k+1]) in op order, null writes already removed.  The
// state left behind is chains_absorb_kernel's, so the calls mix freely on one
// mirsha_chains.
__global__ __launch_bounds__(kBlockThreads) void chains_commit_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ act,
    const uint32_t* __restrict__ efirst, uint32_t n_active, uint32_t* __restrict__ h, uint32_t* __restrict__ pend,
    uint64_t* __restrict__ cnt, uint8_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t c = valid ? act[k] : 0u;
    uint32_t e = valid ? efirst[k] : 0u;
    const uint32_t end = valid ? efirst[k + 1] : 0u;
    uint32_t st[8], pw[8];
    uint64_t n = 0;
    if (valid) chain_state_load(h, pend, cnt, c, st, pw, n);
    commit_walk(digests, ent, e, end, st, pw, n, out);
    if (valid) chain_state_store(h, pend, cnt, c, st, pw, n);
}

// One lane per segment of the cycle's commit programme
// (mirsha_commit_seg_plan): segment s runs entries ent[sfirst[s] ..
// sfirst[s+1]) of chain seg_chain[s].  What differs from chains_commit_kernel:
// a lane that is not its chain's FIRST segment loads no state (it starts from
// Hasher()), one that is not the LAST stores none, and the wave raises its
// issue priority once at entry (seg_prio): it is one latency-bound wave meant
// to run beside a saturating request launch whose waves run at priorities up
// to 3.  No atomics, no waiting; the only cross-lane dependence is the ballot
// that keeps the walk wave-uniform.
//
// FIRST lanes read h_in / pend_in / cnt_in, LAST lanes write h / pend / cnt.
// The two are the same arrays unless a chain's FIRST and LAST segment lie in
// different waves: a LAST lane's store could then overtake the FIRST lane's
// load, and the host passes a copy of the states taken ahead of the launch.
__global__ __launch_bounds__(kBlockThreads) void chains_commit_seg_kernel(
    const uint8_t* __restrict__ digests, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ seg_chain,
    const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ seg_flags, uint32_t n_seg, const uint32_t* h_in,
    const uint32_t* pend_in, const uint64_t* cnt_in, uint32_t* h, uint32_t* pend, uint64_t* cnt, uint4* out,
    uint32_t prio) {
    seg_prio(prio);
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool valid = k < n_seg;
    const uint32_t c = valid ? seg_chain[k] : 0u;
    const uint32_t flags = valid ? seg_flags[k] : 0u;
    uint32_t e = valid ? sfirst[k] : 0u;
    const uint32_t end = valid ? sfirst[k + 1] : 0u;
    uint32_t st[8], pw[8];
    uint64_t n = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[i] = kH0[i];
        pw[i] = 0u;
    }
    if (flags & MIRSHA_COMMIT_SEG_FIRST) chain_state_load(h_in, pend_in, cnt_in, c, st, pw, n);
    commit_walk(digests, ent, e, end, st, pw, n, reinterpret_cast<uint8_t*>(out));
    if (flags & MIRSHA_COMMIT_SEG_LAST) chain_state_store(h, pend, cnt, c, st, pw, n);
}

namespace {

// The SHA-256 row of chain_kernels: h u32[8 n], pend u32[8 n].
void chains_h0(void* h) { memcpy(h, kH0, sizeof(kH0)); }

constexpr uint32_t chain_grid(uint32_t lanes) { return (lanes + kBlockThreads - 1u) / kBlockThreads; }

hipError_t launch_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                const uint32_t* efirst, uint32_t n_active, void* h, void* pend, uint64_t* cnt,
                                uint8_t* out, int /*variant*/, hipStream_t s, uint64_t* /*pair_launches*/) {
    if (n_active == 0) return hipSuccess;
    launch_k(chains_commit_kernel, chain_grid(n_active), kBlockThreads, 0, s, digests, ent, act, efirst, n_active,
             static_cast<uint32_t*>(h), static_cast<uint32_t*>(pend), cnt, out);
    return hipGetLastError();
}

hipError_t launch_chains_absorb(const uint8_t* digests, const uint32_t* pos, const uint32_t* act, const uint32_t* afirst,
                                uint32_t n_active, void* h, void* pend, uint64_t* cnt, hipStream_t s) {
    if (n_active == 0) return hipSuccess;
    launch_k(chains_absorb_kernel, chain_grid(n_active), kBlockThreads, 0, s, digests, pos, act, afirst, n_active,
             static_cast<uint32_t*>(h), static_cast<uint32_t*>(pend), cnt);
    return hipGetLastError();
}

hipError_t launch_chains_sum(const uint32_t* which, uint32_t k, const void* h, const void* pend, const uint64_t* cnt,
                             uint8_t* out, hipStream_t s) {
    if (k == 0) return hipSuccess;
    launch_k(chains_sum_kernel, chain_grid(k), kBlockThreads, 0, s, which, k, static_cast<const uint32_t*>(h),
             static_cast<const uint32_t*>(pend), cnt, out);
    return hipGetLastError();
}

hipError_t launch_chains_reset(const uint32_t* which, uint32_t k, void* h, uint64_t* cnt, hipStream_t s) {
    if (k == 0) return hipSuccess;
    launch_k(chains_reset_kernel, chain_grid(k), kBlockThreads, 0, s, which, k, static_cast<uint32_t*>(h), cnt);
    return hipGetLastError();
}

hipError_t launch_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                    const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg, const void* h_in,
                                    const void* pend_in, const uint64_t* cnt_in, void* h, void* pend, uint64_t* cnt,
                                    uint8_t* out, uint32_t prio, int /*variant*/, hipStream_t s,
                                    uint64_t* /*pair_launches*/) {
    if (n_seg == 0) return hipSuccess;
    launch_k(chains_commit_seg_kernel, chain_grid(n_seg), kBlockThreads, 0, s, digests, ent, seg_chain, sfirst,
             seg_flags, n_seg, static_cast<const uint32_t*>(h_in), static_cast<const uint32_t*>(pend_in), cnt_in,
             static_cast<uint32_t*>(h), static_cast<uint32_t*>(pend), cnt, reinterpret_cast<uint4*>(out), prio);
    return hipGetLastError();
}

}  // namespace

const ChainKernels& chain_kernels(int hasher) {
    static const ChainKernels sha256 = {32u, 32u, chains_h0, launch_chains_commit, launch_chains_absorb,
                                        launch_chains_sum, launch_chains_reset, launch_chains_commit_seg};
    static const ChainKernels sha512_256 = {64u, 96u, sha512_chains_h0, launch_sha512_chains_commit, nullptr,
                                            launch_sha512_chains_sum, launch_sha512_chains_reset,
                                            launch_sha512_chains_commit_seg};
    return hasher == MIRSHA_HASHER_SHA512_256 ? sha512_256 : sha256;
}

}  // namespace mirsha

namespace mirsha_api {

namespace {

static_assert(mirsha::kCommitEntryCheckpoint == MIRSHA_COMMIT_ENTRY_CHECKPOINT, "plan entry flag");

int chains_which(mirsha_ctx* c, mirsha_chains* ch, const uint32_t* which, uint32_t k) {
    if (!which) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (ch->device != c->device) return fail(c, MIRSHA_EINVAL, "chains belong to another device");
    for (uint32_t j = 0; j < k; j++)
        if (which[j] >= ch->n) return fail(c, MIRSHA_EINVAL, "which[%u] = %u >= %u", j, which[j], ch->n);
    if (int rc = use_device(c)) return rc;
    if (int rc = owner_order(c, ch->ring)) return rc;
    HIP_TRY(c, ch->d_which.ensure(4ull * k));
    HIP_TRY(c, hipMemcpyAsync(ch->d_which.p, which, 4ull * k, hipMemcpyHostToDevice, c->stream));
    return MIRSHA_OK;
}

// What mirsha_chains_commit and mirsha_chains_commit_submit share of their
// checks.  commit_args: the argument checks of a call with ops.
// commit_plan_failed: the message of a plan's refusal (rc, bad op).
int commit_args(mirsha_ctx* c, const mirsha_chains* ch, const uint8_t* digests, bool on_device, uint32_t n_digests,
                const uint32_t* op_chain, const uint32_t* op_digest) {
    if (!op_chain || !op_digest) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (n_digests && !digests) return fail(c, MIRSHA_EINVAL, "NULL digest table (%u digests)", n_digests);
    if (on_device && (reinterpret_cast<uintptr_t>(digests) & 15u))
        return fail(c, MIRSHA_EINVAL, "d_digests must be 16-byte aligned");
    if (ch->device != c->device) return fail(c, MIRSHA_EINVAL, "chains belong to another device");
    return MIRSHA_OK;
}

int commit_plan_failed(mirsha_ctx* c, int rc, uint32_t bad, const mirsha_chains* ch, uint32_t n_digests,
                       const uint32_t* op_chain, const uint32_t* op_digest) {
    if (bad == UINT32_MAX) return fail(c, rc, "commit plan failed");
    if (op_chain[bad] >= ch->n) return fail(c, rc, "op_chain[%u] = %u >= %u", bad, op_chain[bad], ch->n);
    return fail(c, rc, "op_digest[%u] = %u >= %u", bad, op_digest[bad], n_digests);
}

// Both forms of mirsha_chains_commit: the plan (every check, on the host,
// before anything is queued), the digest table (uploaded once if it is host
// memory), the plan block in one copy, one launch, the values back.
int chains_commit(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* digests, bool on_device, uint32_t n_digests,
                  const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint8_t* values_out,
                  uint32_t* n_values_out) {
    if (!c || !ch || !n_values_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    if (n_ops == 0) return MIRSHA_OK;
    if (int r = commit_args(c, ch, digests, on_device, n_digests, op_chain, op_digest)) return r;
    const uint32_t cap = std::min(n_ops, ch->n);  // active chains at most
    const size_t o_first = cap, o_ent = 2ull * cap + 1u;
    ch->plan.resize(o_ent + n_ops);
    uint32_t* plan = ch->plan.data();
    uint32_t na = 0, entries = 0, values = 0, bad = UINT32_MAX;
    const int rc = mirsha_commit_plan(op_chain, op_digest, n_ops, ch->n, n_digests, plan, plan + o_first, plan + o_ent,
                                      &na, &entries, &values, &bad);
    if (rc == MIRSHA_ERANGE)
        return fail(c, rc, "%u ops / %u digests > %u", n_ops, n_digests, MIRSHA_COMMIT_ENTRY_CHECKPOINT);
    if (rc != MIRSHA_OK) return commit_plan_failed(c, rc, bad, ch, n_digests, op_chain, op_digest);
    if (values && !values_out) return fail(c, MIRSHA_EINVAL, "NULL values_out (%u checkpoints)", values);
    if (na == 0) return MIRSHA_OK;  // null writes only
    if (int r = use_device(c)) return r;
    if (int r = owner_order(c, ch->ring)) return r;
    const uint8_t* d_dig = digests;
    if (!on_device && n_digests) {
        HIP_TRY(c, ch->d_dig.ensure(32ull * n_digests));
        HIP_TRY(c, hipMemcpyAsync(ch->d_dig.p, digests, 32ull * n_digests, hipMemcpyHostToDevice, c->stream));
        d_dig = ch->d_dig.as<uint8_t>();
    }
    const size_t plan_bytes = 4ull * (o_ent + entries);
    HIP_TRY(c, ch->d_plan.ensure(plan_bytes));
    HIP_TRY(c, ch->d_out.ensure(32ull * values));
    HIP_TRY(c, hipMemcpyAsync(ch->d_plan.p, plan, plan_bytes, hipMemcpyHostToDevice, c->stream));
    const uint32_t* d_plan = ch->d_plan.as<uint32_t>();
    if (int r = timed_launch(c, 1, [&] {
            return mirsha::chain_kernels(ch->hasher).commit(d_dig, d_plan + o_ent, d_plan, d_plan + o_first, na,
                                                            ch->d_h.p, ch->d_pend.p, ch->d_cnt.as<uint64_t>(),
                                                            ch->d_out.as<uint8_t>(), c->variant, c->stream,
                                                            &ch->pair_launches);
        }))
        return r;
    if (values) HIP_TRY(c, hipMemcpyAsync(values_out, ch->d_out.p, 32ull * values, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // ch->plan and the caller's table feed async copies
    *n_values_out = values;
    return MIRSHA_OK;
}

// Both forms of mirsha_chains_commit_submit: every check and the plan (into
// the context's scratch; a failure leaves the ring as it was), then the segment
// ticket's slot lifecycle (seg_submit, mirsha_ctx.h).
int commit_submit(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* digests, bool on_device, uint32_t n_digests,
                  const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint8_t* values_out,
                  uint32_t* n_values_out, uint64_t* ticket_out) {
    if (!c || !ch || !n_values_out || !ticket_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    const auto t0 = Clock::now();
    SegTicket t;
    uint32_t na = 0, entries = 0;
    const size_t o_pfirst = n_ops, o_pflags = 2ull * n_ops + 1u, o_pent = 3ull * n_ops + 1u;  // in c->cm_plan
    if (n_ops) {
        if (int rc = commit_args(c, ch, digests, on_device, n_digests, op_chain, op_digest)) return rc;
        if (n_ops > MIRSHA_COMMIT_ENTRY_CHECKPOINT || n_digests > MIRSHA_COMMIT_ENTRY_CHECKPOINT)
            return fail(c, MIRSHA_ERANGE, "%u ops / %u digests > %u", n_ops, n_digests, MIRSHA_COMMIT_ENTRY_CHECKPOINT);
        if (c->cm_plan.size() < o_pent + n_ops) c->cm_plan.resize(o_pent + n_ops);
        uint32_t* plan = c->cm_plan.data();
        uint32_t bad = UINT32_MAX;
        const int rc = mirsha_commit_seg_plan(op_chain, op_digest, n_ops, ch->n, n_digests, plan, plan + o_pfirst,
                                              plan + o_pflags, plan + o_pent, &t.n_seg, &na, &entries, &t.values, &bad);
        if (rc != MIRSHA_OK) return commit_plan_failed(c, rc, bad, ch, n_digests, op_chain, op_digest);
        if (t.values && !values_out) return fail(c, MIRSHA_EINVAL, "NULL values_out (%u checkpoints)", t.values);
        t.seg_flags = plan + o_pflags;
    }
    // The slot's block: [seg_chain | sfirst | seg_flags | ent | pad to 16 | host table].
    const uint64_t ns = t.n_seg, o_first = 4ull * ns, o_flags = o_first + 4ull * (ns + 1u), o_ent = o_flags + 4ull * ns;
    const uint64_t o_tab = align16(o_ent + 4ull * entries);
    const mirsha::ChainKernels& kern = mirsha::chain_kernels(ch->hasher);
    t.owner = &ch->ring;
    t.on_device = on_device;
    t.stage_bytes = o_tab + (on_device ? 0ull : 32ull * n_digests);
    t.state[0] = {ch->d_h.p, (uint64_t)kern.h_bytes * ch->n};
    t.state[1] = {ch->d_pend.p, (uint64_t)kern.pend_bytes * ch->n};
    t.state[2] = {ch->d_cnt.p, 8ull * ch->n};
    t.values_out = values_out;
    t.timer = 1;
    return seg_submit(
        c, t, t0,
        [&](uint8_t* st) {
            const uint32_t* plan = c->cm_plan.data();
            memcpy(st, plan, 4ull * ns);
            memcpy(st + o_first, plan + o_pfirst, 4ull * (ns + 1u));
            memcpy(st + o_flags, plan + o_pflags, 4ull * ns);
            memcpy(st + o_ent, plan + o_pent, 4ull * entries);
            if (!on_device && n_digests) memcpy(st + o_tab, digests, 32ull * n_digests);
        },
        // state_in[0..3): where FIRST lanes read h / pend / cnt (the chains'
        // arrays or the ticket's snapshot of them)
        [&](const uint8_t* dv, const uint8_t* const* state_in, uint8_t* rows, hipStream_t q) {
            return kern.commit_seg(on_device ? digests : dv + o_tab, reinterpret_cast<const uint32_t*>(dv + o_ent),
                                   reinterpret_cast<const uint32_t*>(dv), reinterpret_cast<const uint32_t*>(dv + o_first),
                                   reinterpret_cast<const uint32_t*>(dv + o_flags), t.n_seg, state_in[0], state_in[1],
                                   reinterpret_cast<const uint64_t*>(state_in[2]), ch->d_h.p, ch->d_pend.p,
                                   ch->d_cnt.as<uint64_t>(), rows, commit_seg_prio(), c->variant, q,
                                   &ch->pair_launches);
        },
        n_values_out, ticket_out);
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

int mirsha_chains_create_hasher(mirsha_ctx* c, uint32_t n, int hasher, mirsha_chains** out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = nullptr;
    if (hasher != MIRSHA_HASHER_SHA256 && hasher != MIRSHA_HASHER_SHA512_256)
        return fail(c, MIRSHA_EINVAL, "unknown hasher %d", hasher);
    if (n == 0) return fail(c, MIRSHA_EINVAL, "n_chains must be > 0");
    if (int rc = use_device(c)) return rc;
    auto* ch = new mirsha_chains();
    ch->device = c->device;
    ch->n = n;
    ch->hasher = hasher;
    // Hasher() for every chain: H0 as the state's own words, one row replicated.
    const mirsha::ChainKernels& kern = mirsha::chain_kernels(hasher);
    const uint64_t h_bytes = (uint64_t)kern.h_bytes * n, pend_bytes = (uint64_t)kern.pend_bytes * n;
    std::vector<uint8_t> h0(h_bytes);
    kern.h0(h0.data());
    for (uint32_t i = 1; i < n; i++) memcpy(h0.data() + (uint64_t)kern.h_bytes * i, h0.data(), kern.h_bytes);
    auto up = [&]() -> int {
        HIP_TRY(c, ch->d_h.ensure(h_bytes));
        HIP_TRY(c, ch->d_pend.ensure(pend_bytes));
        HIP_TRY(c, ch->d_cnt.ensure(8ull * n));
        HIP_TRY(c, hipMemcpyAsync(ch->d_h.p, h0.data(), h_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(ch->d_pend.p, 0, pend_bytes, c->stream));
        HIP_TRY(c, hipMemsetAsync(ch->d_cnt.p, 0, 8ull * n, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return MIRSHA_OK;
    };
    if (int rc = up()) {
        mirsha_chains_destroy(ch);
        return rc;
    }
    *out = ch;
    return MIRSHA_OK;
}

int mirsha_chains_create(mirsha_ctx* c, uint32_t n, mirsha_chains** out) {
    return mirsha_chains_create_hasher(c, n, MIRSHA_HASHER_SHA256, out);
}

int mirsha_chains_hasher(const mirsha_chains* ch) { return ch ? ch->hasher : MIRSHA_EINVAL; }

int mirsha_chains_pair_launches(const mirsha_chains* ch, uint64_t* out) {
    if (!ch || !out) return MIRSHA_EINVAL;
    *out = ch->pair_launches;
    return MIRSHA_OK;
}

void mirsha_chains_destroy(mirsha_chains* ch) {
    if (!ch) return;
    (void)hipSetDevice(ch->device);
    owner_retire(ch->ring);
    for (DevBuf* b : {&ch->d_h, &ch->d_pend, &ch->d_cnt, &ch->d_dig, &ch->d_pos, &ch->d_act, &ch->d_afirst,
                      &ch->d_which, &ch->d_out, &ch->d_plan})
        b->release();
    delete ch;
}

int mirsha_chains_absorb(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* digests, const uint32_t* chain_of,
                         uint32_t m) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    if (!c || !ch) return MIRSHA_EINVAL;
    if (m == 0) return MIRSHA_OK;
    if (!digests || !chain_of) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (ch->device != c->device) return fail(c, MIRSHA_EINVAL, "chains belong to another device");
    const mirsha::ChainKernels& kern = mirsha::chain_kernels(ch->hasher);
    if (!kern.absorb && m > MIRSHA_COMMIT_ENTRY_CHECKPOINT)  // the writes run as plan entries
        return fail(c, MIRSHA_ERANGE, "%u digests > %u", m, MIRSHA_COMMIT_ENTRY_CHECKPOINT);
    // Group the writes by chain, keeping their order (counting sort).
    std::vector<uint32_t> count(ch->n + 1, 0);
    for (uint32_t i = 0; i < m; i++) {
        if (chain_of[i] >= ch->n) return fail(c, MIRSHA_EINVAL, "chain_of[%u] = %u >= %u", i, chain_of[i], ch->n);
        count[chain_of[i] + 1]++;
    }
    std::vector<uint32_t> act, afirst(1, 0);
    for (uint32_t k = 0; k < ch->n; k++)
        if (count[k + 1]) {
            act.push_back(k);
            afirst.push_back(afirst.back() + count[k + 1]);
        }
    for (uint32_t k = 0; k < ch->n; k++) count[k + 1] += count[k];
    std::vector<uint32_t> pos(m);
    for (uint32_t i = 0; i < m; i++) pos[count[chain_of[i]]++] = i;
    if (int rc = use_device(c)) return rc;
    if (int rc = owner_order(c, ch->ring)) return rc;
    const uint32_t na = (uint32_t)act.size();
    HIP_TRY(c, ch->d_dig.ensure(32ull * m));
    HIP_TRY(c, ch->d_pos.ensure(4ull * m));
    HIP_TRY(c, ch->d_act.ensure(4ull * na));
    HIP_TRY(c, ch->d_afirst.ensure(4ull * (na + 1)));
    HIP_TRY(c, hipMemcpyAsync(ch->d_dig.p, digests, 32ull * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ch->d_pos.p, pos.data(), 4ull * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ch->d_act.p, act.data(), 4ull * na, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ch->d_afirst.p, afirst.data(), 4ull * (na + 1), hipMemcpyHostToDevice, c->stream));
    if (int rc = timed_launch(c, 1, [&] {
            const uint8_t* dig = ch->d_dig.as<uint8_t>();
            const uint32_t *d_pos = ch->d_pos.as<uint32_t>(), *d_act = ch->d_act.as<uint32_t>();
            const uint32_t* d_afirst = ch->d_afirst.as<uint32_t>();
            uint64_t* cnt = ch->d_cnt.as<uint64_t>();
            if (kern.absorb) return kern.absorb(dig, d_pos, d_act, d_afirst, na, ch->d_h.p, ch->d_pend.p, cnt, c->stream);
            // a commit programme without checkpoints: pos = the entries
            return kern.commit(dig, d_pos, d_act, d_afirst, na, ch->d_h.p, ch->d_pend.p, cnt, nullptr, c->variant,
                               c->stream, &ch->pair_launches);
        }))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // host vectors above feed async copies
    return MIRSHA_OK;
}

int mirsha_chains_sum(mirsha_ctx* c, mirsha_chains* ch, const uint32_t* which, uint32_t k, uint8_t* out) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    if (!c || !ch) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (!out) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (int rc = chains_which(c, ch, which, k)) return rc;
    HIP_TRY(c, ch->d_out.ensure(32ull * k));
    if (int rc = timed_launch(c, 1, [&] {
            return mirsha::chain_kernels(ch->hasher).sum(ch->d_which.as<uint32_t>(), k, ch->d_h.p, ch->d_pend.p,
                                                         ch->d_cnt.as<uint64_t>(), ch->d_out.as<uint8_t>(), c->stream);
        }))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(out, ch->d_out.p, 32ull * k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

int mirsha_chains_reset(mirsha_ctx* c, mirsha_chains* ch, const uint32_t* which, uint32_t k) {
    if (!c || !ch) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = chains_which(c, ch, which, k)) return rc;
    if (int rc = timed_launch(c, 1, [&] {
            return mirsha::chain_kernels(ch->hasher).reset(ch->d_which.as<uint32_t>(), k, ch->d_h.p,
                                                           ch->d_cnt.as<uint64_t>(), c->stream);
        }))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

int mirsha_chains_commit(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* digests, uint32_t n_digests,
                         const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint8_t* values_out,
                         uint32_t* n_values_out) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    return chains_commit(c, ch, digests, false, n_digests, op_chain, op_digest, n_ops, values_out, n_values_out);
}

int mirsha_chains_commit_device(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* d_digests, uint32_t n_digests,
                                const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops,
                                uint8_t* values_out, uint32_t* n_values_out) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    return chains_commit(c, ch, d_digests, true, n_digests, op_chain, op_digest, n_ops, values_out, n_values_out);
}

int mirsha_chains_commit_submit(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* digests, uint32_t n_digests,
                                const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops,
                                uint8_t* values_out, uint32_t* n_values_out, uint64_t* ticket_out) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    return commit_submit(c, ch, digests, false, n_digests, op_chain, op_digest, n_ops, values_out, n_values_out,
                         ticket_out);
}

int mirsha_chains_commit_submit_device(mirsha_ctx* c, mirsha_chains* ch, const uint8_t* d_digests, uint32_t n_digests,
                                       const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops,
                                       uint8_t* values_out, uint32_t* n_values_out, uint64_t* ticket_out) {
    if (int rc = chains_hasher_match(c, ch, __func__)) return rc;
    return commit_submit(c, ch, d_digests, true, n_digests, op_chain, op_digest, n_ops, values_out, n_values_out,
                         ticket_out);
}

}  // extern "C"
