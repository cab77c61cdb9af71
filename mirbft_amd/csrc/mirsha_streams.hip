// mirsha_streams.hip — streaming SHA-256 states on the device: Write / Sum /
// Reset over any bytes (mirsha_streams_*, include/mirsha.h; the kernel's
// contract is in mirsha_streams.h).  The hash.Hash boundary of the reference
// (`type Hasher func() hash.Hash`, processor.go:21) and an application log
// that writes more than whole digests (Log.Apply / Log.Snap,
// processor.go:28-31).  A translation unit of its own, as
// mirsha_chains.hip: the hashing kernels keep their code object.
#include "mirsha_ctx.h"
#include "mirsha_streams.h"

namespace mirsha {

// One lane per active stream: the lane loads its stream's row, walks the
// stream's whole programme (StreamLane, mirsha_streams.h) and stores the row.
__global__ __launch_bounds__(kStreamWave) void streams_kernel(
    const uint32_t* __restrict__ arena_words, uint32_t shift, uint32_t span, const uint32_t* __restrict__ act,
    const uint4* __restrict__ ent, uint32_t n_active, uint4* __restrict__ state, uint4* __restrict__ out) {
    const uint32_t* efirst = act + n_active;
    const uint32_t k = blockIdx.x * kStreamWave + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t s = valid ? act[k] : 0u;
    StreamLane ln;
    ln.fresh(valid ? efirst[k] : 0u, valid ? efirst[k + 1] : 0u);
    // one row of kStateQuads per stream, one address for the load and the store
    uint4* const row = state + (uint64_t)kStateQuads * s;
    if (valid) ln.load_row(row);
    const StreamArgs a = {buffer_rsrc(arena_words, span), span, shift, ent};
    ln.start(a);
    while (__ballot(ln.live()) != 0ull) ln.step(a, out);
    if (valid) ln.store_row(row);
}

hipError_t launch_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                          const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s) {
    if (n_active == 0) return hipSuccess;
    const uint32_t grid = (n_active + kStreamWave - 1u) / kStreamWave;
    launch_k(streams_kernel, grid, kStreamWave, 0, s, arena_words, shift, span, act, reinterpret_cast<const uint4*>(ent),
             n_active, reinterpret_cast<uint4*>(state), reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

}  // namespace mirsha

namespace mirsha_api {

namespace {

constexpr uint32_t kStateBytes = MIRSHA_STREAM_STATE_BYTES;
constexpr uint32_t kRowWords = mirsha::kStreamStateBytes / 4u;  // a stream's row on the device
const uint8_t kStateMagic[4] = {'s', 'h', 'a', 3};

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
inline uint32_t get_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// Both forms of mirsha_streams_run.  Order: every check and the plan (on the
// host, before anything is queued), the block in one copy, one launch, the
// values back, one synchronisation.
int streams_run(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, bool on_device, uint64_t arena_len,
                const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off, const uint32_t* op_len,
                uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    if (!c || !st || !n_values_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    if (n_ops == 0) return MIRSHA_OK;
    StreamPrep p;
    p.arena = arena, p.on_device = on_device, p.arena_len = arena_len;
    if (int r = streams_prepare(c, st, false, op_stream, op_kind, op_off, op_len, n_ops, values_out, &p)) return r;
    const uint32_t na = p.n_active;
    if (na == 0) return MIRSHA_OK;  // zero-length writes only
    if (int r = use_device(c)) return r;
    if (int r = owner_order(c, st->ring)) return r;
    // [act | efirst | pad to 16 | entry records | packed bytes (host form)]
    const uint64_t o_first = 4ull * na, o_ent = align16(o_first + 4ull * (na + 1u)), o_bytes = o_ent + 16ull * p.entries;
    const uint64_t h2d = o_bytes + (on_device ? 0ull : p.bytes);
    HIP_TRY(c, st->stage.ensure(h2d));
    HIP_TRY(c, st->dev.ensure(h2d + kArenaSlack));  // the last word of the bytes lies inside
    HIP_TRY(c, st->d_out.ensure(32ull * std::max(p.values, 1u)));
    uint8_t* sg = st->stage.as<uint8_t>();
    p.pack(st, sg + o_ent, sg + o_bytes);
    memcpy(sg, st->act.data(), 4ull * na);
    memcpy(sg + o_first, st->efirst.data(), 4ull * (na + 1u));
    HIP_TRY(c, hipMemcpyAsync(st->dev.p, sg, h2d, hipMemcpyHostToDevice, c->stream));
    const uint8_t* dv = st->dev.as<uint8_t>();
    p.window(dv + o_bytes);
    if (int r = timed_launch(c, kTimerStreams, [&] {
            return mirsha::launch_streams(p.words, p.shift, p.span, reinterpret_cast<const uint32_t*>(dv),
                                          reinterpret_cast<const uint32_t*>(dv + o_ent), na, st->d_state.as<uint8_t>(),
                                          st->d_out.as<uint8_t>(), c->stream);
        }))
        return r;
    if (p.values)
        HIP_TRY(c, hipMemcpyAsync(values_out, st->d_out.p, 32ull * p.values, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_values_out = p.values;
    return MIRSHA_OK;
}

int streams_which(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, const void* rows) {
    if (!which || !rows) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (st->device != c->device) return fail(c, MIRSHA_EINVAL, "streams belong to another device");
    for (uint32_t j = 0; j < k; j++)
        if (which[j] >= st->n) return fail(c, MIRSHA_EINVAL, "which[%u] = %u >= %u", j, which[j], st->n);
    return use_device(c);
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

int mirsha_streams_create(mirsha_ctx* c, uint32_t n, mirsha_streams** out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = nullptr;
    if (n == 0) return fail(c, MIRSHA_EINVAL, "n_streams must be > 0");
    if (int rc = use_device(c)) return rc;
    auto* st = new mirsha_streams();
    st->device = c->device;
    st->n = n;
    constexpr uint32_t kWords = mirsha::kStreamStateBytes / 4u;
    std::vector<uint32_t> rows((size_t)kWords * n, 0u);  // Hasher(): H0, nothing buffered, count 0
    for (uint32_t i = 0; i < n; i++)
        for (int j = 0; j < 8; j++) rows[(size_t)kWords * i + j] = mirsha::kH0[j];
    auto up = [&]() -> int {
        HIP_TRY(c, st->d_state.ensure(4ull * rows.size()));
        HIP_TRY(c, hipMemcpyAsync(st->d_state.p, rows.data(), 4ull * rows.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return MIRSHA_OK;
    };
    if (int rc = up()) {
        mirsha_streams_destroy(st);
        return rc;
    }
    *out = st;
    return MIRSHA_OK;
}

void mirsha_streams_destroy(mirsha_streams* st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    owner_retire(st->ring);
    for (DevBuf* b : {&st->d_state, &st->dev, &st->d_out}) b->release();
    st->stage.release();
    delete st;
}

int mirsha_streams_run(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, uint64_t arena_len,
                       const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                       const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    if (int rc = sha256_only(c, __func__)) return rc;
    return streams_run(c, st, arena, false, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_run_device(mirsha_ctx* c, mirsha_streams* st, const uint8_t* d_arena, uint64_t arena_len,
                              const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                              const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    if (int rc = sha256_only(c, __func__)) return rc;
    return streams_run(c, st, d_arena, true, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_export(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, uint8_t* out) {
    if (int rc = sha256_only(c, __func__)) return rc;
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, out)) return rc;
    if (int rc = owner_order(c, st->ring)) return rc;
    std::vector<uint32_t> rows((size_t)kRowWords * k);
    for (uint32_t j = 0; j < k; j++)
        HIP_TRY(c, hipMemcpyAsync(&rows[(size_t)kRowWords * j], st->d_state.as<uint32_t>() + (uint64_t)kRowWords * which[j],
                                  4u * kRowWords, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t* r = &rows[(size_t)kRowWords * j];  // [h 8 | block 16 | count lo, hi | 0, 0]
        uint8_t* row = out + (uint64_t)kStateBytes * j;
        memcpy(row, kStateMagic, 4);
        for (int i = 0; i < 8; i++) put_be32(row + 4 + 4 * i, r[i]);
        const uint32_t fill = r[24] & 63u;
        for (int i = 0; i < 16; i++) put_be32(row + 36 + 4 * i, r[8 + i]);
        memset(row + 36 + fill, 0, 64u - fill);  // behind the fill the block's words are stale
        put_be32(row + 100, r[25]);
        put_be32(row + 104, r[24]);
    }
    return MIRSHA_OK;
}

int mirsha_streams_import(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, const uint8_t* in) {
    if (int rc = sha256_only(c, __func__)) return rc;
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, in)) return rc;
    if (int rc = owner_order(c, st->ring)) return rc;
    for (uint32_t j = 0; j < k; j++)
        if (memcmp(in + (uint64_t)kStateBytes * j, kStateMagic, 4) != 0)
            return fail(c, MIRSHA_EINVAL, "state %u does not begin with \"sha\\x03\"", j);
    std::vector<uint32_t> rows((size_t)kRowWords * k, 0u);
    for (uint32_t j = 0; j < k; j++) {
        const uint8_t* row = in + (uint64_t)kStateBytes * j;
        uint32_t* r = &rows[(size_t)kRowWords * j];
        for (int i = 0; i < 8; i++) r[i] = get_be32(row + 4 + 4 * i);
        for (int i = 0; i < 16; i++) r[8 + i] = get_be32(row + 36 + 4 * i);
        r[25] = get_be32(row + 100);
        r[24] = get_be32(row + 104);
        HIP_TRY(c, hipMemcpyAsync(st->d_state.as<uint32_t>() + (uint64_t)kRowWords * which[j], r, 4u * kRowWords,
                                  hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

}  // extern "C"
