// mirsha_device.h — what the .hip units share beyond the compression itself
// (sha256_device.h): the one launch path, the issue priority of the segment
// kernels, the wave-wide max / min, the digest store and the digest-list
// primitives of the dependent-pass kernels.  HIP only: mirsha_host.cpp (plain
// C++) never includes it.
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
// (mirsha_chains.hip, mirsha_streams_ring.hip).  The priority is wave-uniform; readfirstlane keeps
// the branches scalar, so exactly one s_setprio executes (s_setprio ignores
// exec: fixed_prio, mirsha_kernels.hip).
__device__ __forceinline__ void seg_prio(uint32_t p) {
    p = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
    if (p >= 3u) __builtin_amdgcn_s_setprio(3);
    else if (p == 2u) __builtin_amdgcn_s_setprio(2);
    else if (p == 1u) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// ---- wave-wide reductions ------------------------------------------------
// Wave-wide max / min, wave-uniform result (an SGPR).  DPP inside each 16-lane
// row (quad_perm xor 1 / xor 2, row_ror 4 / 8: four VALU ops, no LDS), then
// the four row results by v_readlane and a scalar reduction.  Called with all
// 64 lanes active (every call site is at a kernel's top, before divergence);
// a DPP source outside the row keeps the lane's own value.
// (The DPP moves' "old" operand is the op's identity, so hipcc folds each
// move into the max / min itself: v_max_u32_dpp, one VALU per step.)
template <bool kMax>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v) {
    auto op = [](uint32_t a, uint32_t b) { return kMax ? (a > b ? a : b) : (a < b ? a : b); };
    constexpr int id = kMax ? 0 : -1;
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x124, 0xF, 0xF, false));  // row_ror:4
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x128, 0xF, 0xF, false));  // row_ror:8
    const uint32_t r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_reduce<true>(v); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return wave_reduce<false>(v); }

// ---- digests ----------------------------------------------------------------
// Row `msg` of `out` (16-byte aligned): two plain 128-bit vector stores of the
// byte-swapped state words.
__device__ __forceinline__ void store_digest(uint8_t* out, uint32_t msg, const uint32_t st[8]) {
    uint4* d = reinterpret_cast<uint4*>(out + 32ull * msg);
    d[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]),
                      __builtin_bswap32(st[3]));
    d[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]),
                      __builtin_bswap32(st[7]));
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

// Digest `id` through a range-checked descriptor: a dead slot, and any index
// at or past n_digests whatever its value, reads zeros instead of faulting,
// without a branch.  The row offset is 32 bits, so the index is clamped to
// kMaxListDigests ahead of the multiply: 32 * (2^27 - 1) = 0xFFFFFFE0 lies
// outside every table (n_digests <= 2^27 - 1), where 32 * 2^27 would wrap to
// row 0.  kNullIndex, when a caller passes it as live, clamps there too.
__device__ __forceinline__ void load_digest(__amdgpu_buffer_rsrc_t rsrc, uint32_t id, bool live, uint4& x0,
                                            uint4& x1) {
    const uint32_t o = live ? 32u * min(id, kMaxListDigests) : 0xFFFFFFE0u;
    const auto a = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0);
    const auto b = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + 16u, 0, 0);
    x0 = make_uint4(a[0], a[1], a[2], a[3]);
    x1 = make_uint4(b[0], b[1], b[2], b[3]);
}

}  // namespace mirsha
