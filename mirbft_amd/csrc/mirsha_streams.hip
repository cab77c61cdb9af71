// mirsha_streams.hip — streaming SHA-256 states on the device: Write / Sum /
// Reset over any bytes (mirsha_streams_*, include/mirsha.h; the kernel's
// contract is in mirsha_streams.h).  The hash.Hash boundary of the reference
// (`type Hasher func() hash.Hash`, processor.go:21) and an application log
// that writes more than whole digests (Log.Apply / Log.Snap,
// processor.go:28-31).  A translation unit of its own, as
// mirsha_chains.hip: the hashing kernels keep their code object.
#include "mirsha_ctx.h"
#include "mirsha_sha512_streams.h"
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

namespace {

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
inline uint32_t get_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// The SHA-256 row of stream_kernels.  A device row as u32 words:
// [h 8 | block 16 | count lo, hi | 0, 0] (mirsha_streams.h); an exported state:
// the magic, h as big-endian u32, the buffered bytes zero-padded to 64, the
// length as big-endian u64.
void stream_row0(uint8_t* row) {  // Hasher(): H0, nothing buffered, count 0
    memset(row, 0, kStreamStateBytes);
    memcpy(row, kH0, sizeof(kH0));
}
void stream_pack(const uint8_t* row, uint8_t* out) {
    uint32_t r[kStreamStateBytes / 4u];
    memcpy(r, row, sizeof r);
    for (int i = 0; i < 8; i++) put_be32(out + 4 + 4 * i, r[i]);
    const uint32_t fill = r[24] & 63u;
    for (int i = 0; i < 16; i++) put_be32(out + 36 + 4 * i, r[8 + i]);
    memset(out + 36 + fill, 0, 64u - fill);  // behind the fill the block's words are stale
    put_be32(out + 100, r[25]);
    put_be32(out + 104, r[24]);
}
void stream_unpack(const uint8_t* in, uint8_t* row) {
    uint32_t r[kStreamStateBytes / 4u] = {};
    for (int i = 0; i < 8; i++) r[i] = get_be32(in + 4 + 4 * i);
    for (int i = 0; i < 16; i++) r[8 + i] = get_be32(in + 36 + 4 * i);
    r[25] = get_be32(in + 100);
    r[24] = get_be32(in + 104);
    memcpy(row, r, sizeof r);
}

// The SHA-512/256 row.  A device row as u32 words: [h 8 x (lo, hi) | block 32 |
// count lo, hi | 0, 0] (mirsha_sha512_streams.h); an exported state: the magic,
// h as big-endian u64, the buffered bytes zero-padded to 128, the length as
// big-endian u64.
void sha512_stream_pack(const uint8_t* row, uint8_t* out) {
    uint32_t r[kSha512StreamStateBytes / 4u];
    memcpy(r, row, sizeof r);
    for (int i = 0; i < 8; i++) {
        put_be32(out + 4 + 8 * i, r[2 * i + 1]);
        put_be32(out + 8 + 8 * i, r[2 * i]);
    }
    const uint32_t fill = r[48] & 127u;
    for (int i = 0; i < 32; i++) put_be32(out + 68 + 4 * i, r[16 + i]);
    memset(out + 68 + fill, 0, 128u - fill);
    put_be32(out + 196, r[49]);
    put_be32(out + 200, r[48]);
}
void sha512_stream_unpack(const uint8_t* in, uint8_t* row) {
    uint32_t r[kSha512StreamStateBytes / 4u] = {};
    for (int i = 0; i < 8; i++) {
        r[2 * i + 1] = get_be32(in + 4 + 8 * i);
        r[2 * i] = get_be32(in + 8 + 8 * i);
    }
    for (int i = 0; i < 32; i++) r[16 + i] = get_be32(in + 68 + 4 * i);
    r[49] = get_be32(in + 196);
    r[48] = get_be32(in + 200);
    memcpy(row, r, sizeof r);
}

}  // namespace

const StreamKernels& stream_kernels(int hasher) {
    static const StreamKernels sha256 = {kStreamStateBytes, MIRSHA_STREAM_STATE_BYTES, {'s', 'h', 'a', 3},
                                         stream_row0,       stream_pack,               stream_unpack,
                                         launch_streams,    launch_streams_seg};
    static const StreamKernels sha512_256 = {kSha512StreamStateBytes, MIRSHA_STREAM_STATE_BYTES_SHA512,
                                             {'s', 'h', 'a', 6},      sha512_stream_row0,
                                             sha512_stream_pack,      sha512_stream_unpack,
                                             launch_sha512_streams,   launch_sha512_streams_seg};
    return hasher == MIRSHA_HASHER_SHA512_256 ? sha512_256 : sha256;
}

}  // namespace mirsha

namespace mirsha_api {

namespace {

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
            return mirsha::stream_kernels(st->hasher).run(p.words, p.shift, p.span,
                                                          reinterpret_cast<const uint32_t*>(dv),
                                                          reinterpret_cast<const uint32_t*>(dv + o_ent), na,
                                                          st->d_state.as<uint8_t>(), st->d_out.as<uint8_t>(), c->stream);
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

int mirsha_streams_create_hasher(mirsha_ctx* c, uint32_t n, int hasher, mirsha_streams** out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = nullptr;
    if (hasher != MIRSHA_HASHER_SHA256 && hasher != MIRSHA_HASHER_SHA512_256)
        return fail(c, MIRSHA_EINVAL, "unknown hasher %d", hasher);
    if (n == 0) return fail(c, MIRSHA_EINVAL, "n_streams must be > 0");
    if (int rc = use_device(c)) return rc;
    auto* st = new mirsha_streams();
    st->device = c->device;
    st->n = n;
    st->hasher = hasher;
    const mirsha::StreamKernels& kern = mirsha::stream_kernels(hasher);
    st->row_bytes = kern.row_bytes;
    std::vector<uint8_t> rows((size_t)kern.row_bytes * n);  // Hasher() for every stream: one row replicated
    kern.row0(rows.data());
    for (uint32_t i = 1; i < n; i++) memcpy(rows.data() + (size_t)kern.row_bytes * i, rows.data(), kern.row_bytes);
    auto up = [&]() -> int {
        HIP_TRY(c, st->d_state.ensure(rows.size()));
        HIP_TRY(c, hipMemcpyAsync(st->d_state.p, rows.data(), rows.size(), hipMemcpyHostToDevice, c->stream));
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

int mirsha_streams_create(mirsha_ctx* c, uint32_t n, mirsha_streams** out) {
    return mirsha_streams_create_hasher(c, n, MIRSHA_HASHER_SHA256, out);
}

int mirsha_streams_hasher(const mirsha_streams* st) { return st ? st->hasher : MIRSHA_EINVAL; }

int mirsha_stream_state_bytes(int hasher, uint32_t* bytes_out) {
    if (hasher != MIRSHA_HASHER_SHA256 && hasher != MIRSHA_HASHER_SHA512_256) return MIRSHA_EINVAL;
    if (bytes_out) *bytes_out = mirsha::stream_kernels(hasher).export_bytes;
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
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    return streams_run(c, st, arena, false, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_run_device(mirsha_ctx* c, mirsha_streams* st, const uint8_t* d_arena, uint64_t arena_len,
                              const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                              const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    return streams_run(c, st, d_arena, true, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_export(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, uint8_t* out) {
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, out)) return rc;
    if (int rc = owner_order(c, st->ring)) return rc;
    const mirsha::StreamKernels& kern = mirsha::stream_kernels(st->hasher);
    const size_t rb = kern.row_bytes;
    std::vector<uint8_t> rows(rb * k);
    for (uint32_t j = 0; j < k; j++)
        HIP_TRY(c, hipMemcpyAsync(&rows[rb * j], st->d_state.as<uint8_t>() + rb * which[j], rb, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < k; j++) {
        uint8_t* row = out + (uint64_t)kern.export_bytes * j;
        memcpy(row, kern.magic, 4);
        kern.pack(&rows[rb * j], row);
    }
    return MIRSHA_OK;
}

int mirsha_streams_import(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, const uint8_t* in) {
    if (int rc = streams_hasher_match(c, st, __func__)) return rc;
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, in)) return rc;
    if (int rc = owner_order(c, st->ring)) return rc;
    const mirsha::StreamKernels& kern = mirsha::stream_kernels(st->hasher);
    for (uint32_t j = 0; j < k; j++)
        if (memcmp(in + (uint64_t)kern.export_bytes * j, kern.magic, 4) != 0)
            return fail(c, MIRSHA_EINVAL, "state %u does not begin with \"sha\\x%02x\"", j, kern.magic[3]);
    const size_t rb = kern.row_bytes;
    std::vector<uint8_t> rows(rb * k);
    for (uint32_t j = 0; j < k; j++) {
        kern.unpack(in + (uint64_t)kern.export_bytes * j, &rows[rb * j]);
        HIP_TRY(c, hipMemcpyAsync(st->d_state.as<uint8_t>() + rb * which[j], &rows[rb * j], rb, hipMemcpyHostToDevice,
                                  c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

}  // extern "C"
