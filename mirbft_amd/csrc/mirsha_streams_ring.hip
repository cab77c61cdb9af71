// mirsha_streams_ring.hip — a stream programme on the asynchronous ring
// (mirsha_streams_submit / _submit_device, include/mirsha.h): the ring form of
// mirsha_streams_run, as mirsha_chains_commit_submit is the ring form of
// mirsha_chains_commit (mirsha_chains.hip).  With it an application log that writes any bytes
// (StreamLog) has its commit stage beside the hash stage (commitInParallel,
// processor.go:447-470).  A translation unit of its own: the hashing kernels
// keep their code object, and the synchronous mirsha_streams_run keeps its
// kernel.  Both stream kernels walk a programme by the same step (StreamLane,
// mirsha_streams.h).
#include "mirsha_ctx.h"
#include "mirsha_streams.h"

namespace mirsha {

// One lane per segment of the programme (mirsha_stream_seg_plan): segment k
// runs entries [sfirst[k], sfirst[k+1]) of stream seg_stream[k].  What differs
// from streams_kernel: a lane that is not its stream's FIRST segment loads no
// row (it starts from Hasher(): H0, count 0, a zero block, so its first window
// lies at its first write's own offset), one that is not the LAST stores none,
// and the wave sets its issue priority once at entry (seg_prio).  The value
// rows are the step's two plain 128-bit vector stores: `out` may be
// host-visible page-locked memory.  No atomics, no waiting; the only
// cross-lane dependence is the ballot that keeps the loop wave-uniform.
//
// FIRST lanes read state_in, LAST lanes write state.  The two are the same
// array unless a stream's FIRST and LAST segment lie in different waves: a
// LAST lane's store could then overtake the FIRST lane's load, and the host
// passes a copy of the rows taken ahead of the launch.
__global__ __launch_bounds__(kStreamWave) void streams_seg_kernel(
    const uint32_t* __restrict__ arena_words, uint32_t shift, uint32_t span, const uint32_t* __restrict__ seg_stream,
    const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ seg_flags, const uint4* __restrict__ ent,
    uint32_t n_seg, const uint4* state_in, uint4* state, uint4* out, uint32_t prio) {
    seg_prio(prio);
    const uint32_t k = blockIdx.x * kStreamWave + threadIdx.x;
    const bool valid = k < n_seg;
    const uint32_t s = valid ? seg_stream[k] : 0u;
    const uint32_t flags = valid ? seg_flags[k] : 0u;
    StreamLane ln;
    ln.fresh(valid ? sfirst[k] : 0u, valid ? sfirst[k + 1] : 0u);
    if (flags & MIRSHA_STREAM_SEG_FIRST) ln.load_row(state_in + (uint64_t)kStateQuads * s);
    const StreamArgs a = {buffer_rsrc(arena_words, span), span, shift, ent};
    ln.start(a);
    while (__ballot(ln.live()) != 0ull) ln.step(a, out);
    if (flags & MIRSHA_STREAM_SEG_LAST) ln.store_row(state + (uint64_t)kStateQuads * s);
}

hipError_t launch_streams_seg(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* seg_stream,
                              const uint32_t* sfirst, const uint32_t* seg_flags, const uint32_t* ent, uint32_t n_seg,
                              const uint8_t* state_in, uint8_t* state, uint8_t* out, uint32_t prio, hipStream_t s) {
    if (n_seg == 0) return hipSuccess;
    const uint32_t grid = (n_seg + kStreamWave - 1u) / kStreamWave;
    launch_k(streams_seg_kernel, grid, kStreamWave, 0, s, arena_words, shift, span, seg_stream, sfirst, seg_flags,
             reinterpret_cast<const uint4*>(ent), n_seg, reinterpret_cast<const uint4*>(state_in),
             reinterpret_cast<uint4*>(state), reinterpret_cast<uint4*>(out), prio);
    return hipGetLastError();
}

}  // namespace mirsha

namespace mirsha_api {

int streams_prepare(mirsha_ctx* c, mirsha_streams* st, bool segments, const uint32_t* op_stream, const uint32_t* op_kind,
                    const uint64_t* op_off, const uint32_t* op_len, uint32_t n_ops, const uint8_t* values_out,
                    StreamPrep* p) {
    if (!op_stream || !op_kind) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (st->device != c->device) return fail(c, MIRSHA_EINVAL, "streams belong to another device");
    if (p->on_device && p->arena_len > MIRSHA_MAX_DEVICE_ARENA_BYTES)
        return fail(c, MIRSHA_ERANGE, "device arena of %llu bytes > %u", (unsigned long long)p->arena_len,
                    MIRSHA_MAX_DEVICE_ARENA_BYTES);
    if (n_ops <= MIRSHA_STREAM_MAX_OPS) {  // (above it the plan refuses before it writes)
        if (segments) {
            st->seg_stream.resize(n_ops);
            st->sfirst.resize((size_t)n_ops + 1u);
            st->seg_flags.resize(n_ops);
        } else {
            st->act.resize(std::min(n_ops, st->n));  // active streams at most
            st->efirst.resize(st->act.size() + 1u);
        }
        st->kind.resize(n_ops);
        st->len.resize(n_ops);
        st->off.resize(n_ops);
    }
    uint32_t bad = UINT32_MAX;
    const int rc =
        segments ? mirsha_stream_seg_plan(op_stream, op_kind, op_off, op_len, n_ops, st->n, p->arena_len, 0,
                                          st->seg_stream.data(), st->sfirst.data(), st->seg_flags.data(),
                                          st->kind.data(), st->off.data(), st->len.data(), &p->n_seg, &p->n_active,
                                          &p->entries, &p->values, &p->bytes, &bad)
                 : mirsha_stream_plan(op_stream, op_kind, op_off, op_len, n_ops, st->n, p->arena_len, 0, st->act.data(),
                                      st->efirst.data(), st->kind.data(), st->off.data(), st->len.data(), &p->n_active,
                                      &p->entries, &p->values, &p->bytes, &bad);
    if (rc == MIRSHA_ERANGE) return fail(c, rc, "%u ops > %u", n_ops, MIRSHA_STREAM_MAX_OPS);
    if (rc != MIRSHA_OK) {
        if (bad == UINT32_MAX) return fail(c, rc, "stream plan failed (a NULL op array?)");
        if (op_stream[bad] >= st->n) return fail(c, rc, "op_stream[%u] = %u >= %u", bad, op_stream[bad], st->n);
        if (op_kind[bad] > MIRSHA_STREAM_RESET) return fail(c, rc, "op_kind[%u] = %u is no kind", bad, op_kind[bad]);
        return fail(c, rc, "op %u writes [%llu, +%u) of an arena of %llu bytes", bad, (unsigned long long)op_off[bad],
                    op_len[bad], (unsigned long long)p->arena_len);
    }
    if (p->bytes && !p->arena)
        return fail(c, MIRSHA_EINVAL, "NULL arena (%llu bytes to write)", (unsigned long long)p->bytes);
    if (p->values && !values_out) return fail(c, MIRSHA_EINVAL, "NULL values_out (%u sums)", p->values);
    if (!p->on_device) {  // what crosses PCIe: every distinct range once (mirsha_stream_plan, pack)
        st->poff.resize(n_ops);
        p->bytes = mirsha::host::stream_pack_offsets(st->off.data(), st->len.data(), p->entries, st->poff.data());
        if (p->bytes + kArenaSlack > MIRSHA_MAX_DEVICE_ARENA_BYTES)
            return fail(c, MIRSHA_ERANGE, "%llu written bytes > %u", (unsigned long long)p->bytes,
                        MIRSHA_MAX_DEVICE_ARENA_BYTES - (uint32_t)kArenaSlack);
    }
    return MIRSHA_OK;
}

void StreamPrep::pack(mirsha_streams* st, uint8_t* rec8, uint8_t* packed) const {
    if (!on_device) {
        uint64_t at = 0;
        for (uint32_t e = 0; e < entries; e++) {
            if (st->len[e] && st->poff[e] == at) {  // the range's first entry: its bytes go in here
                memcpy(packed + at, arena + st->off[e], st->len[e]);
                at += st->len[e];
            }
            st->off[e] = st->poff[e];
        }
    }
    uint32_t* rec = reinterpret_cast<uint32_t*>(rec8);  // the plan's entry arrays, one 16-byte record each
    for (uint32_t e = 0; e < entries; e++) {
        rec[4ull * e] = st->kind[e];
        rec[4ull * e + 1] = st->len[e];
        rec[4ull * e + 2] = (uint32_t)st->off[e];
        rec[4ull * e + 3] = (uint32_t)(st->off[e] >> 32);
    }
}

// Aligned words only: a word never crosses a page, so the up to 3 bytes beside
// a device arena that share a word with it are safe to load.
void StreamPrep::window(const uint8_t* d_packed) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(on_device ? arena : d_packed);
    const uint64_t extent = on_device ? arena_len : bytes;
    shift = (uint32_t)(base & 3u);
    span = extent ? (uint32_t)((shift + extent + 3u) & ~3ull) : 0u;
    words = reinterpret_cast<const uint32_t*>(base - shift);
}

namespace {

// Both forms of mirsha_streams_submit: every check and the plan (into the
// object's scratch; a failure leaves the ring as it was), then the segment
// ticket's slot lifecycle (seg_submit, mirsha_ctx.h).
int streams_submit(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, bool on_device, uint64_t arena_len,
                   const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off, const uint32_t* op_len,
                   uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out, uint64_t* ticket_out) {
    if (!c || !st || !n_values_out || !ticket_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    const auto t0 = Clock::now();
    StreamPrep p;
    p.arena = arena, p.on_device = on_device, p.arena_len = arena_len;
    if (n_ops)
        if (int rc = streams_prepare(c, st, true, op_stream, op_kind, op_off, op_len, n_ops, values_out, &p)) return rc;
    // The slot's block: [seg_stream | sfirst | seg_flags | pad to 16 | entry records | packed bytes (host form)].
    const uint64_t ns = p.n_seg, o_first = 4ull * ns, o_flags = o_first + 4ull * (ns + 1u);
    const uint64_t o_ent = align16(o_flags + 4ull * ns), o_bytes = o_ent + 16ull * p.entries;
    SegTicket t;
    t.owner = &st->ring;
    t.on_device = on_device;
    t.seg_flags = st->seg_flags.data();
    t.n_seg = p.n_seg;
    t.stage_bytes = o_bytes + (on_device ? 0ull : p.bytes);
    t.dev_slack = kArenaSlack;  // the last word of the bytes lies inside
    t.state[0] = {st->d_state.p, (uint64_t)st->row_bytes * st->n};
    t.values_out = values_out;
    t.values = p.values;
    t.timer = kTimerStreams;
    return seg_submit(
        c, t, t0,
        [&](uint8_t* sg) {
            p.pack(st, sg + o_ent, sg + o_bytes);
            memcpy(sg, st->seg_stream.data(), 4ull * ns);
            memcpy(sg + o_first, st->sfirst.data(), 4ull * (ns + 1u));
            memcpy(sg + o_flags, st->seg_flags.data(), 4ull * ns);
        },
        [&](const uint8_t* dv, const uint8_t* const* state_in, uint8_t* rows, hipStream_t q) {
            p.window(dv + o_bytes);
            return mirsha::stream_kernels(st->hasher).seg(
                p.words, p.shift, p.span, reinterpret_cast<const uint32_t*>(dv),
                reinterpret_cast<const uint32_t*>(dv + o_first), reinterpret_cast<const uint32_t*>(dv + o_flags),
                reinterpret_cast<const uint32_t*>(dv + o_ent), p.n_seg, state_in[0], st->d_state.as<uint8_t>(), rows,
                commit_seg_prio(), q);
        },
        n_values_out, ticket_out);
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

int mirsha_streams_submit(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, uint64_t arena_len,
                          const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                          const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                          uint64_t* ticket_out) {
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    return streams_submit(c, st, arena, false, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                          n_values_out, ticket_out);
}

int mirsha_streams_submit_device(mirsha_ctx* c, mirsha_streams* st, const uint8_t* d_arena, uint64_t arena_len,
                                 const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                                 const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                                 uint64_t* ticket_out) {
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    return streams_submit(c, st, d_arena, true, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                          n_values_out, ticket_out);
}

}  // extern "C"
