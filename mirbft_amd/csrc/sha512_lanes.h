// sha512_lanes.h — the per-lane bodies of the SHA-512/256 kernels, shared by
// the two units that hold them: mirsha_sha512.hip (the request kernel and the
// list walk of the hash, verify and ring calls) and mirsha_sha512_plan.hip (the
// kernels of the device plans).  A kernel is one call of a lane function; each
// is __forceinline__, so every kernel keeps its registers to itself.
// Everything that decides bytes is sha512_device.h (proved on the CPU); this
// file adds the loaders.  No lane function uses LDS, atomics or waiting; lanes
// depend on each other only through a block loop's ballot.  HIP only.
#pragma once
#include "mirsha_device.h"
#include "sha512_device.h"

namespace mirsha {

// 256 threads (4 waves, one per SIMD), as every other kernel of the library.
// Occupancy: __launch_bounds__(256) alone (no minimum-waves argument) lets the
// compiler take what the 80 unrolled rounds need: 168 to 174 VGPRs by kernel
// (2 or 3 waves per SIMD), no scratch.  Asking for 4 waves (128 VGPRs) spilled
// 37 VGPRs to scratch.  A form of the rounds that fits 160 VGPRs (3 waves; Maj
// as a bit-select, 276 more VALU a block) measured 6 % slower on 2^20 x 272 B:
// the rounds are VALU-bound and the shorter stream wins (DESIGN.md §1.6,
// profiles/hasher, profiles/hasher_plan).
constexpr uint32_t kSha512Threads = 256;

// Offset of every load of a lane that has nothing to read: beyond any
// descriptor's range (records <= kMaxBufferArena = 0xFFFFFF00 rounded up to a
// word), with room for a block's 132 bytes before the offset wraps.  The range
// check turns such loads into zeros without a memory access.
constexpr uint32_t kDeadOffset = 0xFFFFFF00u;

// The 33 aligned dwords that cover the 128-byte block at arena byte `addr`
// (aligned down to 4 bytes; v_perm resolves addr & 3 later).
struct RawBlock {
    uint32_t v[33];
};

// The range check covers a whole access: a 128-bit load that straddles the
// end of the arena returns zero for its in-range dwords too.  So a block whose
// 132 bytes do not all lie below `records` (the arena's last block, one lane
// of a launch) takes 33 single-dword loads, each checked on its own; kNoMerge
// keeps hipcc from merging them back into wide loads.
__device__ __forceinline__ void issue_block(__amdgpu_buffer_rsrc_t rsrc, uint32_t records, uint32_t addr, bool active,
                                            RawBlock& r) {
    const uint32_t a = active ? (addr & ~3u) : kDeadOffset;
    if (!active || (uint64_t)a + 132u <= records) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, a + 16u * q, 0, 0);
            r.v[4 * q] = v[0]; r.v[4 * q + 1] = v[1]; r.v[4 * q + 2] = v[2]; r.v[4 * q + 3] = v[3];
        }
        r.v[32] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, a + 128u, 0, 0);
    } else {
#pragma unroll
        for (int k = 0; k < 33; k++) r.v[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, a + 4u * k, 0, kNoMerge);
    }
}

// Row `row` of `out` (16-byte aligned): the digest of the state, two plain
// 128-bit vector stores.
__device__ __forceinline__ void store_sha512_digest(uint8_t* out, uint32_t row, const uint64_t st[8]) {
    uint32_t d[8];
    sha512::digest_words(st, d);
    uint4* r = reinterpret_cast<uint4*>(out + 32ull * row);
    r[0] = make_uint4(d[0], d[1], d[2], d[3]);
    r[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// Lane `slot` hashes message order[slot] (order == NULL: identity).  The block
// loop is wave-uniform and runs to the wave's largest block count; a lane that
// is finished idles (its loads take the dead offset, its rounds are skipped).
// Correct for any order; the callers' bucket order (sorted by 64-byte block
// count, so monotone in length) keeps a tile's 128-byte block counts within
// one of each other.  Block b + 1's loads are issued before block b's rounds.
__device__ __forceinline__ void sha512_msg_lane(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                const uint32_t* __restrict__ order, uint32_t n,
                                                uint8_t* __restrict__ out, uint32_t slot) {
    const bool valid = slot < n;
    const uint32_t msg = valid ? (order ? order[slot] : slot) : 0u;
    const uint32_t L = valid ? len[msg] : 0u;
    const uint32_t o = valid ? (uint32_t)off[msg] : 0u;
    const uint32_t nb = valid ? sha512::blocks_for_len(L) : 0u;
    const uint32_t records = (uint32_t)((arena_len + 3u) & ~3ull);
    const __amdgpu_buffer_rsrc_t rsrc = buffer_rsrc(arena, records);
    const uint32_t sel = be_sel(o & 3u);  // every block of the message starts at the same addr & 3
    uint64_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    RawBlock raw;
    issue_block(rsrc, records, o, 0u < nb, raw);
    for (uint32_t blk = 0; __ballot(blk < nb) != 0ull; blk++) {
        uint32_t bw[32];
#pragma unroll
        for (int k = 0; k < 32; k++) bw[k] = be_word(raw.v[k + 1], raw.v[k], sel);
        issue_block(rsrc, records, o + 128u * (blk + 1u), blk + 1u < nb, raw);
        if (blk < nb) {
            const uint32_t p = 128u * blk;
            if ((uint64_t)p + 128u > L) sha512::pad_block(bw, p, L, blk + 1u == nb);
            uint64_t w[16];
            sha512::join_words(bw, w);
            sha512::compress(st, w);
        }
    }
    if (valid) store_sha512_digest(out, msg, st);
}

// The next (up to) four non-null rows of a lane's list from entry e on.
struct ListRows {
    uint32_t rows[4][8];
    uint32_t filled;  // < 4: the list ends in this block
};

__device__ __forceinline__ void keep_row(uint32_t row[8], const uint4& x0, const uint4& x1) {
    row[0] = x0.x; row[1] = x0.y; row[2] = x0.z; row[3] = x0.w;
    row[4] = x1.x; row[5] = x1.y; row[6] = x1.z; row[7] = x1.w;
}

// Skips MIRSHA_NULL_INDEX entries (they contribute nothing), four index loads
// at a time; then requests the rows.  Index loads are range-checked against
// n_entries and row loads against n_digests (an index in [n_digests,
// kNullIndex) reads zeros whatever its value: load_digest clamps it ahead of
// the 32-bit row offset, as for hash_list).  !live: no entry is read, every
// load takes a dead offset.
// The row ids are kept by selects, never by a dynamic register index.
__device__ __forceinline__ void fetch_rows(__amdgpu_buffer_rsrc_t drs, __amdgpu_buffer_rsrc_t irs, uint32_t& e,
                                           uint32_t e1, bool live, ListRows& r) {
    uint32_t id[4] = {0u, 0u, 0u, 0u};
    uint32_t filled = 0u;
    while (live && filled < 4u && e < e1) {
        uint32_t v[4];
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = ld_u32(irs, 4u * (e + (uint32_t)s), e + (uint32_t)s < e1);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool here = e < e1 && filled < 4u;  // entry e = v[s] is this block's to look at
            const bool take = here && v[s] != kNullIndex;
#pragma unroll
            for (int j = 0; j < 4; j++) id[j] = (take && filled == (uint32_t)j) ? v[s] : id[j];
            filled += take ? 1u : 0u;
            e += here ? 1u : 0u;
        }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        uint4 x0, x1;
        load_digest(drs, id[s], (uint32_t)s < filled, x0, x1);
        keep_row(r.rows[s], x0, x1);
    }
    r.filled = filled;
}

// Dependent pass, lane k: message k = concat(digests[idx[e]] for e in [first[k],
// first[k + 1])) without its MIRSHA_NULL_INDEX entries; the empty list (or one
// of nulls only) is the digest of the empty message.  Which entries a block
// takes never depends on a hash value, so block b + 1's rows are fetched
// before block b's rounds.
__device__ __forceinline__ void sha512_list_lane(const uint8_t* __restrict__ digests, uint32_t n_digests,
                                                 const uint32_t* __restrict__ idx, uint32_t n_entries,
                                                 const uint32_t* __restrict__ first, uint32_t n_lists,
                                                 uint8_t* __restrict__ out, uint32_t k) {
    const __amdgpu_buffer_rsrc_t drs = buffer_rsrc(digests, 32u * n_digests);
    const __amdgpu_buffer_rsrc_t irs = buffer_rsrc(idx, 4u * n_entries);
    const bool valid = k < n_lists;
    uint32_t e = valid ? first[k] : 0u;
    const uint32_t e1 = valid ? first[k + 1] : 0u;
    uint64_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    ListRows cur;
    fetch_rows(drs, irs, e, e1, valid, cur);
    bool more = valid;  // this lane has a block to hash
    for (uint32_t d0 = 0; __ballot(more) != 0ull; d0 += 4u) {
        const bool last = cur.filled < 4u;
        ListRows nxt;
        fetch_rows(drs, irs, e, e1, more && !last, nxt);
        if (more) {
            uint64_t w[16];
            sha512::list_block(cur.rows, d0, d0 + cur.filled, last, w);
            sha512::compress(st, w);
        }
        more = more && !last;
        cur = nxt;
    }
    if (valid) store_sha512_digest(out, k, st);
}

// The four rows of block b of a plan's list: a plan's lists are compacted at
// creation (no MIRSHA_NULL_INDEX entry), so block b takes entries e0 + 4 b + s,
// s < 4, live while 4 b + s < c: no null test, no data-dependent loop.
// kUniform: identity lists, the row IS the entry, so no index is loaded.  Index
// loads are range-checked against n_entries and row loads against n_digests;
// an inactive load takes a dead offset and reads zeros.
template <bool kUniform>
__device__ __forceinline__ void plan_rows(__amdgpu_buffer_rsrc_t drs, __amdgpu_buffer_rsrc_t irs, uint32_t e0,
                                          uint32_t c, uint32_t b, bool live, uint32_t rows[4][8]) {
    uint32_t id[4];
    bool on[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t ord = 4u * b + (uint32_t)s;
        on[s] = live && ord < c;
        id[s] = kUniform ? e0 + ord : ld_u32(irs, 4u * (e0 + ord), on[s]);
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        uint4 x0, x1;
        load_digest(drs, id[s], on[s], x0, x1);
        keep_row(rows[s], x0, x1);
    }
}

// The dependent pass of a plan, lane k: list k of the compacted lists has
// c = cfirst[k + 1] - cfirst[k] rows and exactly c / 4 + 1 blocks (32 c mod 128
// is never >= 112: the final block always has room for the padding; the empty
// list is the one block of the empty message).  The block loop is wave-uniform
// to the wave's largest count; block b + 1's index and row loads are issued
// before block b's 80 rounds.  kUniform (`uniform` = B > 0: identity lists of B
// entries, uniform_lists() in mirsha_plan.hip): e0 = k B, c = min(B, n_entries
// - k B), row = e0 + 4 b + s; cidx and cfirst are not read.
template <bool kUniform>
__device__ __forceinline__ void sha512_plan_list_lane(const uint8_t* __restrict__ digests, uint32_t n_digests,
                                                      const uint32_t* __restrict__ cidx, uint32_t n_entries,
                                                      const uint32_t* __restrict__ cfirst, uint32_t n_lists,
                                                      uint32_t uniform, uint8_t* __restrict__ out, uint32_t k) {
    const __amdgpu_buffer_rsrc_t drs = buffer_rsrc(digests, 32u * n_digests);
    const __amdgpu_buffer_rsrc_t irs = buffer_rsrc(cidx, 4u * n_entries);
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
    uint64_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha512::kH0[i];
    uint32_t cur[4][8];
    plan_rows<kUniform>(drs, irs, e0, c, 0u, valid, cur);
    for (uint32_t b = 0; __ballot(b < nb) != 0ull; b++) {
        uint32_t nxt[4][8];
        plan_rows<kUniform>(drs, irs, e0, c, b + 1u, b + 1u < nb, nxt);
        if (b < nb) {
            uint64_t w[16];
            sha512::list_block(cur, 4u * b, c, b + 1u == nb, w);
            sha512::compress(st, w);
        }
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int i = 0; i < 8; i++) cur[s][i] = nxt[s][i];
    }
    if (valid) store_sha512_digest(out, k, st);
}

}  // namespace mirsha
