// mirsha_sha512_streams.hip — the streaming hash states of the second hasher,
// SHA-512/256: Write / Sum / Reset over any bytes when the node's Hasher is
// sha512.New512_256 (processor.go:21,58).  Two kernels and nothing else:
//
//   sha512_streams_kernel      one lane per active stream: a call's programme
//                              (mirsha_streams_run / _run_device)
//   sha512_streams_seg_kernel  one lane per segment of a stream ticket
//                              (mirsha_streams_submit / _submit_device)
//
// A translation unit and code object of its own, as mirsha_sha512_chains.hip.
// What decides bytes (the plan of a step, the merge, the padding) is
// sha512_stream.h, proved on the CPU; this file adds the loader and the walk.
// No LDS, no atomics, no waiting; lanes depend on each other only through the
// walk's ballot.  The state's row and the window's bounds: mirsha_sha512_streams.h.
#include "mirsha_sha512_streams.h"

#include <cstring>

#include "../../include/mirsha.h"
#include "mirsha_device.h"
#include "mirsha_streams.h"
#include "sha512_stream.h"

namespace mirsha {

static_assert(sha512::kStreamWrite == MIRSHA_STREAM_WRITE && sha512::kStreamSum == MIRSHA_STREAM_SUM &&
                  sha512::kStreamSumReset == MIRSHA_STREAM_SUM_RESET && sha512::kStreamReset == MIRSHA_STREAM_RESET,
              "entry kinds");
static_assert(kSha512StreamStateBytes % 16u == 0u, "a row is a whole number of 16-byte accesses");

constexpr uint32_t kSha512StateQuads = kSha512StreamStateBytes / 16u;

// The 33 aligned words that hold the 128-byte window at arena offset a (mod
// 2^32), as load_window (mirsha_streams.h): a word at or above `span` and every
// word of a lane that is not writing takes ld_u32's dead offset.  Single
// aligned 4-byte loads: a wider load that straddles the range's end would read
// zero for its in-range words too.
__device__ __forceinline__ void load_window512(__amdgpu_buffer_rsrc_t rs, uint32_t span, bool wr, uint32_t a,
                                               uint32_t d[sha512::kStreamWindowWords]) {
    const uint32_t a0 = a & ~3u;
#pragma unroll
    for (int i = 0; i < sha512::kStreamWindowWords; i++) {
        const uint32_t o = a0 + 4u * (uint32_t)i;
        d[i] = ld_u32(rs, o, wr && o < span);
    }
}

// A pointer held in the lane's own registers from here on.  The rounds keep up
// to 80 SGPRs of round constants live (sha512::compress), which leaves too few
// for every wave-uniform address of the walk: without this the compiler parks
// `out` and the rows' base in a VGPR's lanes (SGPR spills) and fetches them
// back every step.  There is room in the VGPRs.  A register constraint on an
// empty statement, as MIRSHA512_K_FENCE: no instruction is emitted.
template <class T>
__device__ __forceinline__ T* lane_held(T* p) {
    asm volatile("" : "+v"(p));
    return p;
}

// What a launch's lanes share: the arena's descriptor.
struct Sha512StreamArgs {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t span, shift;
};

// A lane's walk over entries [e, end) of one stream, as StreamLane
// (mirsha_streams.h) with the step of sha512_stream.h: straight-line steps,
// the rounds run on every lane when any lane's step has a compression, and the
// only divergent branch inside a step guards the row's store.  The walk runs
// one step ahead of the hashing: the window is merged into the block first, so
// d[] is dead while the next step's window (and the entry behind the next) is
// requested, ahead of this step's 80 rounds.
struct Sha512StreamLane {
    uint64_t st[8], hs[8];
    uint32_t bw[32];
    sha512::StreamWalk wk;
    const uint4* ep;  // the lane's current entry; its last one once the lane is done
    uint32_t left;    // entries from *ep to the lane's end; 0: the lane is done
    uint4 x, xn;
    uint32_t d[sha512::kStreamWindowWords];

    // Hasher() -- H0, count 0, an all-zero block -- before entries [e0, e1).
    __device__ __forceinline__ void fresh(const uint4* ent, uint32_t e0, uint32_t e1) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            st[i] = sha512::kH0[i];
            hs[i] = 0ull;
        }
#pragma unroll
        for (int i = 0; i < 32; i++) bw[i] = 0u;
        wk.n = 0ull;
        wk.pos = 0u;
        wk.sum2 = 0u;
        ep = ent + e0;
        left = e1 - e0;
    }

    __device__ __forceinline__ void load_row(const uint4* row) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 v = row[q];
            st[2 * q] = (uint64_t)v.y << 32 | v.x;
            st[2 * q + 1] = (uint64_t)v.w << 32 | v.z;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint4 v = row[4 + q];
            bw[4 * q] = v.x; bw[4 * q + 1] = v.y; bw[4 * q + 2] = v.z; bw[4 * q + 3] = v.w;
        }
        const uint4 v = row[12];
        wk.n = (uint64_t)v.y << 32 | v.x;
    }

    __device__ __forceinline__ void store_row(uint4* row) const {
#pragma unroll
        for (int q = 0; q < 4; q++)
            row[q] = make_uint4((uint32_t)st[2 * q], (uint32_t)(st[2 * q] >> 32), (uint32_t)st[2 * q + 1],
                                (uint32_t)(st[2 * q + 1] >> 32));
#pragma unroll
        for (int q = 0; q < 8; q++) row[4 + q] = make_uint4(bw[4 * q], bw[4 * q + 1], bw[4 * q + 2], bw[4 * q + 3]);
        row[12] = make_uint4((uint32_t)wk.n, (uint32_t)(wk.n >> 32), 0u, 0u);
    }

    __device__ __forceinline__ bool live() const { return left != 0u; }

    // The loads of the step that comes next: the entry behind it and its window.
    __device__ __forceinline__ void request(const Sha512StreamArgs& a) {
        load_window512(a.rs, a.span, left != 0u && (x.x & 3u) == MIRSHA_STREAM_WRITE, wk.window(x.z + a.shift), d);
        xn = ep[left > 1u ? 1u : 0u];
    }

    __device__ __forceinline__ void start(const Sha512StreamArgs& a) {
        x = ep[0];
        request(a);
    }

    __device__ __forceinline__ void step(const Sha512StreamArgs& a, uint4* out) {
        const sha512::StreamStep s = wk.plan(x.x, x.y, left != 0u);
        // x.w, the offset's high word, is 0: span < 2^32
        sha512::stream_merge(bw, d, wk.window(x.z + a.shift) & 3u, s);
        uint64_t w[16], ts[8];
        sha512::stream_block(bw, st, hs, wk.n, s, w, ts);
        // where the lane stands after this step, and the loads of the next one
        wk.advance(s);
        ep += (s.adv && left > 1u) ? 1 : 0;
        left -= s.adv ? 1u : 0u;
        if (s.adv) x = xn;
        request(a);  // d's old values are merged already
        // what the step still needs behind the rounds, in VGPRs (stream_after)
        uint32_t after = sha512::stream_after(s), row = s.row;
        // wave-uniform: skipped when no lane's step has a compression (short writes only)
        if (__ballot(s.full || s.sm) != 0ull) sha512::compress(ts, w);
        if (after & sha512::kStreamFin) {
            uint32_t dw[8];
            sha512::digest_words(ts, dw);
            uint4* o = out + 2ull * row;
            o[0] = make_uint4(dw[0], dw[1], dw[2], dw[3]);
            o[1] = make_uint4(dw[4], dw[5], dw[6], dw[7]);
        }
        sha512::stream_finish(st, hs, ts, after);
    }
};

// One lane per active stream: the lane loads its stream's row, walks the
// stream's whole programme and stores the row (streams_kernel, mirsha_streams.hip).
__global__ __launch_bounds__(kStreamWave) void sha512_streams_kernel(
    const uint32_t* __restrict__ arena_words, uint32_t shift, uint32_t span, const uint32_t* __restrict__ act,
    const uint4* __restrict__ ent, uint32_t n_active, uint4* __restrict__ state, uint4* __restrict__ out) {
    const uint32_t* efirst = act + n_active;
    const uint32_t k = blockIdx.x * kStreamWave + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t s = valid ? act[k] : 0u;
    const uint32_t e1 = valid ? efirst[k + 1] : 0u;
    Sha512StreamLane ln;
    ln.fresh(ent, valid ? efirst[k] : 0u, e1);
    uint4* const row = state + (uint64_t)kSha512StateQuads * s;
    if (valid) ln.load_row(row);
    const Sha512StreamArgs a = {buffer_rsrc(arena_words, span), span, shift};
    uint4* const rows = lane_held(out);
    ln.start(a);
    while (__ballot(ln.live()) != 0ull) ln.step(a, rows);
    // an active stream has an entry, so its lane's range ends above 0: asked of
    // the lane's own register, where `valid` would hold a lane mask across the walk
    if (e1 != 0u) ln.store_row(row);
}

// One lane per segment of the programme (mirsha_stream_seg_plan), as
// streams_seg_kernel (mirsha_streams_ring.hip): a lane that is not its
// stream's FIRST segment starts from Hasher(), only a LAST one stores the state
// it ends in, and the wave takes its issue priority once at entry.  FIRST lanes
// read state_in: the streams' own rows, or the copy of them the host took
// ahead of the launch when a stream's FIRST and LAST segment lie in different
// waves (so the two are not __restrict__).  The value rows are the step's two
// plain 128-bit vector stores: `out` may be host-visible page-locked memory.
__global__ __launch_bounds__(kStreamWave) void sha512_streams_seg_kernel(
    const uint32_t* __restrict__ arena_words, uint32_t shift, uint32_t span, const uint32_t* __restrict__ seg_stream,
    const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ seg_flags, const uint4* __restrict__ ent,
    uint32_t n_seg, const uint4* state_in, uint4* state, uint4* out, uint32_t prio) {
    seg_prio(prio);
    const uint32_t k = blockIdx.x * kStreamWave + threadIdx.x;
    const bool valid = k < n_seg;
    const uint32_t s = valid ? seg_stream[k] : 0u;
    const uint32_t flags = valid ? seg_flags[k] : 0u;
    Sha512StreamLane ln;
    ln.fresh(ent, valid ? sfirst[k] : 0u, valid ? sfirst[k + 1] : 0u);
    if (flags & MIRSHA_STREAM_SEG_FIRST) ln.load_row(state_in + (uint64_t)kSha512StateQuads * s);
    uint4* const row = lane_held(state + (uint64_t)kSha512StateQuads * s);
    uint4* const rows = lane_held(out);
    const Sha512StreamArgs a = {buffer_rsrc(arena_words, span), span, shift};
    ln.start(a);
    while (__ballot(ln.live()) != 0ull) ln.step(a, rows);
    if (flags & MIRSHA_STREAM_SEG_LAST) ln.store_row(row);
}

void sha512_stream_row0(uint8_t* row) {
    memset(row, 0, kSha512StreamStateBytes);
    memcpy(row, sha512::kH0, sizeof(sha512::kH0));
}

hipError_t launch_sha512_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                                 const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s) {
    if (n_active == 0) return hipSuccess;
    const uint32_t grid = (n_active + kStreamWave - 1u) / kStreamWave;
    launch_k(sha512_streams_kernel, grid, kStreamWave, 0, s, arena_words, shift, span, act,
             reinterpret_cast<const uint4*>(ent), n_active, reinterpret_cast<uint4*>(state),
             reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_sha512_streams_seg(const uint32_t* arena_words, uint32_t shift, uint32_t span,
                                     const uint32_t* seg_stream, const uint32_t* sfirst, const uint32_t* seg_flags,
                                     const uint32_t* ent, uint32_t n_seg, const uint8_t* state_in, uint8_t* state,
                                     uint8_t* out, uint32_t prio, hipStream_t s) {
    if (n_seg == 0) return hipSuccess;
    const uint32_t grid = (n_seg + kStreamWave - 1u) / kStreamWave;
    launch_k(sha512_streams_seg_kernel, grid, kStreamWave, 0, s, arena_words, shift, span, seg_stream, sfirst,
             seg_flags, reinterpret_cast<const uint4*>(ent), n_seg, reinterpret_cast<const uint4*>(state_in),
             reinterpret_cast<uint4*>(state), reinterpret_cast<uint4*>(out), prio);
    return hipGetLastError();
}

}  // namespace mirsha
