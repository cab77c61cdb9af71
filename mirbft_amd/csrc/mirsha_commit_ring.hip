// mirsha_commit_ring.hip — a cycle's Commits on the asynchronous ring
// (mirsha_chains_commit_submit / _submit_device, include/mirsha.h): the
// commit stage of ProcessorWorkPool (commitInParallel, processor.go:363-394,
// :447-470) beside its hash stage (mirsha_async.hip).  A translation unit of
// its own, as mirsha_expect.hip: the hashing kernels keep their code object,
// and the synchronous mirsha_chains_commit keeps its kernel.  Both commit
// kernels walk a programme by the same step (CommitStep / commit_fetch,
// mirsha_device.h).
#include "mirsha_ctx.h"

namespace mirsha {

// One lane per segment of the cycle's commit programme
// (mirsha_commit_seg_plan): segment s runs entries ent[sfirst[s] ..
// sfirst[s+1]) of chain seg_chain[s].  What differs from chains_commit_kernel:
// a lane that is not its chain's FIRST segment loads no state (it starts from
// Hasher()), one that is not the LAST stores none, the checkpoint rows are
// plain 128-bit vector stores (`out` may be host-visible page-locked memory),
// and the wave raises its issue priority once at entry (seg_prio): it is one
// latency-bound wave meant to run beside a saturating request launch whose
// waves run at priorities up to 3.  No atomics, no waiting; the only
// cross-lane dependence is the ballot that keeps the loop wave-uniform.
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
    if (flags & MIRSHA_COMMIT_SEG_FIRST) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            st[i] = h_in[8ull * c + i];
            pw[i] = pend_in[8ull * c + i];
        }
        n = cnt_in[c];
    }
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
            uint4* o = out + 2ull * s.row;
            o[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]),
                              __builtin_bswap32(st[3]));
            o[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]),
                              __builtin_bswap32(st[7]));
#pragma unroll
            for (int i = 0; i < 8; i++) st[i] = kH0[i];
        }
        s = nx;
    }
    if (flags & MIRSHA_COMMIT_SEG_LAST) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            h[8ull * c + i] = st[i];
            pend[8ull * c + i] = pw[i];
        }
        cnt[c] = n;
    }
}

hipError_t launch_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                    const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                    const uint32_t* h_in, const uint32_t* pend_in, const uint64_t* cnt_in, uint32_t* h,
                                    uint32_t* pend, uint64_t* cnt, uint8_t* out, uint32_t prio, hipStream_t s) {
    if (n_seg == 0) return hipSuccess;
    const uint32_t grid = (n_seg + kBlockThreads - 1u) / kBlockThreads;
    launch_k(chains_commit_seg_kernel, grid, kBlockThreads, 0, s, digests, ent, seg_chain, sfirst, seg_flags, n_seg, h_in,
             pend_in, cnt_in, h, pend, cnt, reinterpret_cast<uint4*>(out), prio);
    return hipGetLastError();
}

}  // namespace mirsha

namespace mirsha_api {

namespace {

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
    t.owner = &ch->ring;
    t.on_device = on_device;
    t.stage_bytes = o_tab + (on_device ? 0ull : 32ull * n_digests);
    t.state[0] = {ch->d_h.p, chains_h_bytes(ch)};
    t.state[1] = {ch->d_pend.p, chains_pend_bytes(ch)};
    t.state[2] = {ch->d_cnt.p, chains_cnt_bytes(ch)};
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
        [&](const uint8_t* dv, const uint8_t* const* state_in, uint8_t* rows, hipStream_t q) {
            return chains_launch_commit_seg(
                ch, on_device ? digests : dv + o_tab, reinterpret_cast<const uint32_t*>(dv + o_ent),
                reinterpret_cast<const uint32_t*>(dv), reinterpret_cast<const uint32_t*>(dv + o_first),
                reinterpret_cast<const uint32_t*>(dv + o_flags), t.n_seg, state_in, rows, commit_seg_prio(), q);
        },
        n_values_out, ticket_out);
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

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
