// mirsha_streams_ring.hip — a stream programme on the asynchronous ring
// (mirsha_streams_submit / _submit_device, include/mirsha.h): the ring form of
// mirsha_streams_run, as mirsha_commit_ring.hip is the ring form of
// mirsha_chains_commit.  With it an application log that writes any bytes
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

namespace {

// Both forms of mirsha_streams_submit.  Order: every check and the plan (into
// the object's scratch; a failure leaves the ring as it was), then the ring's
// slot lifecycle (mirsha_ctx.h): the slot, the staging copy, the device work
// on the commit stream, the ticket.
int streams_submit(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, bool on_device, uint64_t arena_len,
                   const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off, const uint32_t* op_len,
                   uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out, uint64_t* ticket_out) {
    if (!c || !st || !n_values_out || !ticket_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    auto t0 = Clock::now();
    double ph[MIRSHA_PROF_PHASES] = {};
    uint32_t ns = 0, na = 0, entries = 0, values = 0;
    uint64_t bytes = 0;
    if (n_ops) {
        if (!op_stream || !op_kind) return fail(c, MIRSHA_EINVAL, "NULL argument");
        if (st->device != c->device) return fail(c, MIRSHA_EINVAL, "streams belong to another device");
        if (on_device && arena_len > MIRSHA_MAX_DEVICE_ARENA_BYTES)
            return fail(c, MIRSHA_ERANGE, "device arena of %llu bytes > %u", (unsigned long long)arena_len,
                        MIRSHA_MAX_DEVICE_ARENA_BYTES);
        if (n_ops <= MIRSHA_STREAM_MAX_OPS) {  // (above it the plan refuses before it writes)
            st->seg_stream.resize(n_ops);
            st->sfirst.resize((size_t)n_ops + 1u);
            st->seg_flags.resize(n_ops);
            st->kind.resize(n_ops);
            st->len.resize(n_ops);
            st->off.resize(n_ops);
        }
        uint32_t bad = UINT32_MAX;
        const int rc = mirsha_stream_seg_plan(op_stream, op_kind, op_off, op_len, n_ops, st->n, arena_len, 0,
                                              st->seg_stream.data(), st->sfirst.data(), st->seg_flags.data(),
                                              st->kind.data(), st->off.data(), st->len.data(), &ns, &na, &entries,
                                              &values, &bytes, &bad);
        if (rc == MIRSHA_ERANGE) return fail(c, rc, "%u ops > %u", n_ops, MIRSHA_STREAM_MAX_OPS);
        if (rc != MIRSHA_OK) {
            if (bad == UINT32_MAX) return fail(c, rc, "stream plan failed (a NULL op array?)");
            if (op_stream[bad] >= st->n) return fail(c, rc, "op_stream[%u] = %u >= %u", bad, op_stream[bad], st->n);
            if (op_kind[bad] > MIRSHA_STREAM_RESET)
                return fail(c, rc, "op_kind[%u] = %u is no kind", bad, op_kind[bad]);
            return fail(c, rc, "op %u writes [%llu, +%u) of an arena of %llu bytes", bad,
                        (unsigned long long)op_off[bad], op_len[bad], (unsigned long long)arena_len);
        }
        if (bytes && !arena)
            return fail(c, MIRSHA_EINVAL, "NULL arena (%llu bytes to write)", (unsigned long long)bytes);
        if (values && !values_out) return fail(c, MIRSHA_EINVAL, "NULL values_out (%u sums)", values);
        if (!on_device) {  // what crosses PCIe: every distinct range once (mirsha_stream_plan, pack)
            st->poff.resize(n_ops);
            bytes = mirsha::host::stream_pack_offsets(st->off.data(), st->len.data(), entries, st->poff.data());
            if (bytes + kArenaSlack > MIRSHA_MAX_DEVICE_ARENA_BYTES)
                return fail(c, MIRSHA_ERANGE, "%llu written bytes > %u", (unsigned long long)bytes,
                            MIRSHA_MAX_DEVICE_ARENA_BYTES - (uint32_t)kArenaSlack);
        }
    }
    ph[MIRSHA_PROF_VALIDATE] = ms_since(t0);
    t0 = Clock::now();
    AsyncSlot* slot = nullptr;
    if (int rc = ring_acquire(c, &slot)) return rc;
    AsyncSlot& sl = *slot;
    CommitSlot& cm = sl.cm;
    if (ns) {
        if (!c->xcommit) HIP_TRY(c, hipStreamCreateWithFlags(&c->xcommit, hipStreamNonBlocking));
        if (int rc = ensure_event(c, &st->ev_run)) return rc;
        if (on_device)
            if (int rc = ensure_event(c, &sl.ev_in)) return rc;
    }
    RingQueued queued(c->xcommit);
    // The slot's block: [seg_stream | sfirst | seg_flags | pad to 16 | entry records | packed bytes (host form)].
    const uint64_t o_first = 4ull * ns, o_flags = o_first + 4ull * (ns + 1u), o_ent = align16(o_flags + 4ull * ns);
    const uint64_t o_bytes = o_ent + 16ull * entries;
    const uint64_t h2d = o_bytes + (on_device ? 0ull : bytes);
    const uint64_t state_bytes = (uint64_t)mirsha::kStreamStateBytes * st->n;
    // Does a stream's FIRST segment lie in another wave than its LAST?  Then the
    // FIRST lanes read a copy of the rows taken ahead of the launch.
    bool straddle = false;
    uint8_t* rows = nullptr;
    if (ns) {
        uint32_t first_wave = 0;
        for (uint32_t s = 0; s < ns && !straddle; s++) {
            if (st->seg_flags[s] & MIRSHA_STREAM_SEG_FIRST) first_wave = s / mirsha::kStreamWave;
            if ((st->seg_flags[s] & MIRSHA_STREAM_SEG_LAST) && s / mirsha::kStreamWave != first_wave) straddle = true;
        }
        HIP_TRY(c, cm.stage.ensure(h2d));
        HIP_TRY(c, cm.dev.ensure(h2d + kArenaSlack));  // the last word of the bytes lies inside
        if (straddle) HIP_TRY(c, cm.snap.ensure(state_bytes));
        if (values) {
            // a kernel-writable values_out receives the values from the kernel
            // itself, else the slot's rows do, copied out at retirement
            rows = host_rows(c, values_out);
            if (!rows) {
                HIP_TRY(c, cm.rows.ensure(32ull * values));
                if (int rc = pinned_rows(c, cm.rows, &rows)) return rc;
                sl.retire.rows = SlotRows::kCommit;
                sl.retire.out = values_out;
                sl.retire.n = values;
            }
        }
    }
    ph[MIRSHA_PROF_PLAN] = ms_since(t0);
    t0 = Clock::now();
    auto queue = [&]() -> int {
        uint8_t* sg = cm.stage.as<uint8_t>();
        if (!on_device) {
            uint64_t at = 0;
            for (uint32_t e = 0; e < entries; e++) {
                if (st->len[e] && st->poff[e] == at) {  // the range's first entry: its bytes go in here
                    memcpy(sg + o_bytes + at, arena + st->off[e], st->len[e]);
                    at += st->len[e];
                }
                st->off[e] = st->poff[e];
            }
        }
        memcpy(sg, st->seg_stream.data(), 4ull * ns);
        memcpy(sg + o_first, st->sfirst.data(), 4ull * (ns + 1u));
        memcpy(sg + o_flags, st->seg_flags.data(), 4ull * ns);
        uint32_t* rec = reinterpret_cast<uint32_t*>(sg + o_ent);  // the plan's entry arrays, one 16-byte record each
        for (uint32_t e = 0; e < entries; e++) {
            rec[4ull * e] = st->kind[e];
            rec[4ull * e + 1] = st->len[e];
            rec[4ull * e + 2] = (uint32_t)st->off[e];
            rec[4ull * e + 3] = (uint32_t)(st->off[e] >> 32);
        }
        hipStream_t q = c->xcommit;
        queued.arm();
        if (on_device) {  // the arena is read behind whatever was queued on the context's stream
            HIP_TRY(c, hipEventRecord(sl.ev_in, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(q, sl.ev_in, 0));
        }
        HIP_TRY(c, hipMemcpyAsync(cm.dev.p, sg, h2d, hipMemcpyHostToDevice, q));
        uint8_t* state = st->d_state.as<uint8_t>();
        const uint8_t* state_in = state;
        if (straddle) {
            HIP_TRY(c, hipMemcpyAsync(cm.snap.p, state, state_bytes, hipMemcpyDeviceToDevice, q));
            state_in = cm.snap.as<uint8_t>();
        }
        const uint8_t* dv = cm.dev.as<uint8_t>();
        // aligned words only: a word never crosses a page, so the up to 3 bytes
        // beside a device arena that share a word with it are safe to load
        const uintptr_t base =
            on_device ? reinterpret_cast<uintptr_t>(arena) : reinterpret_cast<uintptr_t>(dv + o_bytes);
        const uint32_t shift = (uint32_t)(base & 3u);
        const uint64_t extent = on_device ? arena_len : bytes;
        const uint32_t span = extent ? (uint32_t)((shift + extent + 3u) & ~3ull) : 0u;
        const uint32_t prio = commit_seg_prio();
        if (int rc = timed_launch(c, kTimerStreams, [&] {
                return mirsha::launch_streams_seg(
                    reinterpret_cast<const uint32_t*>(base - shift), shift, span,
                    reinterpret_cast<const uint32_t*>(dv), reinterpret_cast<const uint32_t*>(dv + o_first),
                    reinterpret_cast<const uint32_t*>(dv + o_flags), reinterpret_cast<const uint32_t*>(dv + o_ent), ns,
                    state_in, state, rows, prio, q);
            }))
            return rc;
        HIP_TRY(c, hipEventRecord(sl.done, q));
        HIP_TRY(c, hipEventRecord(st->ev_run, q));
        return MIRSHA_OK;
    };
    if (ns) {
        if (int rc = queue()) return rc;  // (what it queued is drained: RingQueued)
        st->run_queued = true;
    }
    sl.t_queued = Clock::now();
    ph[MIRSHA_PROF_PACK] = ms_since(t0);
    *n_values_out = values;
    ring_publish(c, sl, queued, ph, ticket_out);
    return MIRSHA_OK;
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

int mirsha_streams_submit(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, uint64_t arena_len,
                          const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                          const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                          uint64_t* ticket_out) {
    return streams_submit(c, st, arena, false, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                          n_values_out, ticket_out);
}

int mirsha_streams_submit_device(mirsha_ctx* c, mirsha_streams* st, const uint8_t* d_arena, uint64_t arena_len,
                                 const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                                 const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                                 uint64_t* ticket_out) {
    return streams_submit(c, st, d_arena, true, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                          n_values_out, ticket_out);
}

}  // extern "C"
