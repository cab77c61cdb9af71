// mirsha_device.h — what the .hip units share beyond the compression itself
// (sha256_device.h): the one launch path, the issue priority of the segment
// kernels, the digest-list primitives of the dependent-pass kernels and the
// step of a commit programme.  HIP only:
// mirsha_host.cpp (plain C++) never includes it.
#pragma once
#include <hip/hip_ext.h>

#include "mirsha_kernels.h"
#include "sha256_device.h"

namespace mirsha {

// ---- launching ------------------------------------------------------------
// Every kernel of the library is launched here: with the thread's pending
// timing events bound to the dispatch (hipExtLaunchKernel) when a timed
// launch set them, else a plain launch.  Errors are left for the caller's
// hipGetLastError, as with <<<...>>>.
template <typename... P, typename... A>
void launch_k(void (*k)(P...), dim3 grid, dim3 block, uint32_t shmem, hipStream_t s, A... args) {
    LaunchEvents& ev = next_launch_events();
    if (ev.start && ev.stop) {
        const hipEvent_t e0 = ev.start, e1 = ev.stop;
        ev = LaunchEvents{};
        hipExtLaunchKernelGGL(k, grid, block, shmem, s, e0, e1, 0u, static_cast<P>(args)...);
    } else {
        k<<<grid, block, shmem, s>>>(static_cast<P>(args)...);
    }
}

// ---- issue priority -------------------------------------------------------
// The wave's issue priority, once at entry of the two segment kernels
// (chains_commit_seg_kernel, mirsha_commit_ring.hip; streams_seg_kernel,
// mirsha_streams_ring.hip).  The priority is wave-uniform; readfirstlane keeps
// the branches scalar, so exactly one s_setprio executes (s_setprio ignores
// exec: fixed_prio, mirsha_kernels.hip).
__device__ __forceinline__ void seg_prio(uint32_t p) {
    p = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
    if (p >= 3u) __builtin_amdgcn_s_setprio(3);
    else if (p == 2u) __builtin_amdgcn_s_setprio(2);
    else if (p == 1u) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// ---- digest lists ---------------------------------------------------------
// 16 raw digest bytes -> 4 big-endian message words (`ends`: the message
// ends right before them, so the 0x80 marker goes into the first).
__device__ __forceinline__ void be_words(const uint4& v, uint32_t w[4], bool ends = false) {
    w[0] = __builtin_bswap32(v.x) | (ends ? 0x80000000u : 0u); w[1] = __builtin_bswap32(v.y);
    w[2] = __builtin_bswap32(v.z); w[3] = __builtin_bswap32(v.w);
}

// One 64-byte block of the message concat(c digests): x = the raw digests of
// ordinals d0 and d0 + 1 (zeros past the end of the list), 0x80 where the
// list ends.  The list's last block also takes list_block_length.
__device__ __forceinline__ void list_block_words(const uint4 x[4], uint32_t d0, uint32_t c, uint32_t w[16]) {
#pragma unroll
    for (int half = 0; half < 2; half++) {
        be_words(x[2 * half], w + 8 * half, d0 + (uint32_t)half == c);
        be_words(x[2 * half + 1], w + 8 * half + 4);
    }
}

// FIPS 180-4 §5.1.1: the 64-bit bit length of an L-byte message, big-endian.
__device__ __forceinline__ void list_block_length(uint32_t w[16], uint32_t L) {
    w[14] = L >> 29;
    w[15] = L << 3;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)bytes, 0x00020000);
}

// Every global read on a chain is an unconditional, range-checked buffer load
// (no branch + wait per element).  aux bit 31 (volatile) keeps hipcc from
// merging adjacent dword loads into a dwordx2/x4, whose range check would
// zero in-range entries that share an access with out-of-range ones at the
// end of the array (lowers to sc0 sc1: L1 bypass, L2-served).
constexpr int kNoMerge = (int)(1u << 31);
__device__ __forceinline__ uint32_t ld_u32(__amdgpu_buffer_rsrc_t rs, uint32_t off, bool live) {
    return __builtin_amdgcn_raw_buffer_load_b32(rs, live ? off : 0xFFFFFFF0u, 0, kNoMerge);
}

// Digest `id` through a range-checked descriptor: a dead slot (or an index
// past n_digests) reads zeros instead of faulting, without a branch.
__device__ __forceinline__ void load_digest(__amdgpu_buffer_rsrc_t rsrc, uint32_t id, bool live, uint4& x0,
                                            uint4& x1) {
    const uint32_t o = live ? 32u * id : 0xFFFFFFE0u;
    const auto a = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0);
    const auto b = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + 16u, 0, 0);
    x0 = make_uint4(a[0], a[1], a[2], a[3]);
    x1 = make_uint4(b[0], b[1], b[2], b[3]);
}

// ---- one step of a commit programme ---------------------------------------
// chains_commit_kernel (mirsha_kernels.hip) and chains_commit_seg_kernel
// (mirsha_commit_ring.hip) walk a lane's programme in these steps.  A step is
// at most one compression: two whole digests (the first may be the digest
// pending from earlier writes), or the final padded block of a checkpoint
// (pending digest, if any, 0x80, bit length: always one block), or a lone
// last write that becomes the pending digest without a compression.
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

}  // namespace mirsha
