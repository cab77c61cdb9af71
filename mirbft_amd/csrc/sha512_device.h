// sha512_device.h — SHA-512/256 (FIPS 180-4 §5.3.6.2, §6.7) for gfx950, one
// message per lane: the second `Hasher` a Processor may be configured with
// (processor.go:21,58; Go's sha512.New512_256).  64-bit words in VGPR pairs:
// a rotate is two v_alignbit_b32, a three-way xor and Maj one v_bitop3_b32 per
// half, Ch one v_bfi_b32 per half, an add one v_lshl_add_u64.
//
// Everything that decides a digest's bytes (the compression, the padding of a
// message's blocks, the blocks of a digest list) is plain C++ and compiles for
// the host as well, so the CPU suite proves it (tests/c/sha512_unit.cpp);
// only the loaders in mirsha_sha512.hip are device code.  The header includes
// nothing of HIP when the compiler is not hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MIRSHA512_HD __host__ __device__ __forceinline__
#else
#define MIRSHA512_HD inline
#endif

namespace mirsha {
namespace sha512 {

#define MIRSHA512_K_TABLE                                                                            \
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,      \
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,      \
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,      \
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,      \
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,      \
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,      \
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,      \
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,      \
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,      \
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,      \
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,      \
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,      \
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,      \
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,      \
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,      \
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,      \
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,      \
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,      \
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,      \
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull

// The round constants.  On the device they live in constant memory, so the
// unrolled rounds fetch them with scalar loads (s_load_dwordx*) instead of
// spending two 32-bit literals per round on the VALU stream; the host reads
// the plain table.
static constexpr uint64_t kK[80] = {MIRSHA512_K_TABLE};
#if defined(__HIP_DEVICE_COMPILE__)
static __constant__ uint64_t kKc[80] = {MIRSHA512_K_TABLE};
#define MIRSHA512_K(j) kKc[(j)]
#else
#define MIRSHA512_K(j) kK[(j)]
#endif

// SHA-512/256's initial hash value (FIPS 180-4 §5.3.6.2).
static constexpr uint64_t kH0[8] = {0x22312194fc2bf72cull, 0x9f555fa3c84c64c2ull, 0x2393b86b6f53b151ull,
                                    0x963877195940eabdull, 0x96283ee2a88effe3ull, 0xbe5e1e2553863992ull,
                                    0x2b0199fc2c85b8aaull, 0x0eb72ddc81c52ca2ull};

constexpr uint32_t kBlockBytes = 128;
constexpr uint32_t kDigestBytes = 32;

// 64-bit pieces on 32-bit VALU.  hipcc lowers a 64-bit rotate by a constant to
// two 64-bit shifts and an or, so the device side spells it out: a rotate is
// two v_alignbit_b32 (alignbit(hi, lo, s) = bits [s, s + 32) of hi:lo), a
// shift one v_alignbit_b32 and one 32-bit shift, a three-way xor one
// v_bitop3_b32 (truth table 0x96) per half.  The host side is the definition.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint64_t join(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
template <int N>
__device__ __forceinline__ uint64_t rotr(uint64_t x) {
    static_assert(N > 0 && N < 64 && N != 32, "rotate amount");
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if constexpr (N < 32)
        return join(__builtin_amdgcn_alignbit(lo, hi, N), __builtin_amdgcn_alignbit(hi, lo, N));
    else
        return join(__builtin_amdgcn_alignbit(hi, lo, N - 32), __builtin_amdgcn_alignbit(lo, hi, N - 32));
}
template <int N>
__device__ __forceinline__ uint64_t shr(uint64_t x) {
    static_assert(N > 0 && N < 32, "shift amount");
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    return join(hi >> N, __builtin_amdgcn_alignbit(hi, lo, N));
}
template <int kTable>
__device__ __forceinline__ uint64_t bitop3(uint64_t a, uint64_t b, uint64_t c) {
    return join(__builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), kTable),
                __builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b, (uint32_t)c, kTable));
}
__device__ __forceinline__ uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) { return bitop3<0x96>(a, b, c); }
// Majority as one op per half (truth table 0xE8; symmetric in its inputs):
// from the bit-select form below hipcc makes four ops per half.
__device__ __forceinline__ uint64_t maj(uint64_t a, uint64_t b, uint64_t c) { return bitop3<0xE8>(a, b, c); }
#else
template <int N>
inline uint64_t rotr(uint64_t x) { return (x >> N) | (x << (64 - N)); }
template <int N>
inline uint64_t shr(uint64_t x) { return x >> N; }
inline uint64_t xor3(uint64_t a, uint64_t b, uint64_t c) { return a ^ b ^ c; }
// Maj = (a ^ b) ? c : b, a bit-select.
inline uint64_t maj(uint64_t a, uint64_t b, uint64_t c) { return ((a ^ b) & c) | (~(a ^ b) & b); }
#endif
MIRSHA512_HD uint64_t bsig0(uint64_t x) { return xor3(rotr<28>(x), rotr<34>(x), rotr<39>(x)); }
MIRSHA512_HD uint64_t bsig1(uint64_t x) { return xor3(rotr<14>(x), rotr<18>(x), rotr<41>(x)); }
MIRSHA512_HD uint64_t ssig0(uint64_t x) { return xor3(rotr<1>(x), rotr<8>(x), shr<7>(x)); }
MIRSHA512_HD uint64_t ssig1(uint64_t x) { return xor3(rotr<19>(x), rotr<61>(x), shr<6>(x)); }
// Ch = e ? f : g, a bit-select: v_bfi_b32 per half.
MIRSHA512_HD uint64_t ch(uint64_t e, uint64_t f, uint64_t g) { return (e & f) | (~e & g); }

// One 128-byte block: st += F(st, w).  w[] holds the 16 big-endian message
// words on entry and is consumed as the rolling 16-word schedule window; 80
// rounds, fully unrolled, every index static.
//
// The round constants come 16 at a time, one group ahead of the rounds that
// use them.  On the device each group's loads hang on a fence that is tied to
// the working state: without it the compiler hoists all 80 loads out of the
// caller's block loop and keeps 160 SGPRs live (it then spilled 96 of them);
// with it 64 are live at most and nothing spills.
#if defined(__HIP_DEVICE_COMPILE__)
#define MIRSHA512_UNROLL _Pragma("unroll")
#define MIRSHA512_K_FENCE(kp, x) asm volatile("" : "+s"(kp), "+v"(x))
// (the constant address space stays in the pointer's type, so the loads behind
// the fence are still scalar loads and not per-lane flat loads)
typedef const uint64_t __attribute__((address_space(4))) * KPtr;
#else
typedef const uint64_t* KPtr;
#define MIRSHA512_UNROLL
#define MIRSHA512_K_FENCE(kp, x) (void)0
#endif
MIRSHA512_HD void compress(uint64_t st[8], uint64_t w[16]) {
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3];
    uint64_t e = st[4], f = st[5], g = st[6], h = st[7];
#define MIRSHA512_ROUND(a, b, c, d, e, f, g, h, j)                                           \
    {                                                                                        \
        if ((j) >= 16)                                                                       \
            w[(j)&15] += ssig1(w[((j)-2) & 15]) + w[((j)-7) & 15] + ssig0(w[((j)-15) & 15]);  \
        const uint64_t t1 = h + bsig1(e) + ch(e, f, g) + kc[(j)&15] + w[(j)&15];             \
        d += t1;                                                                             \
        h = t1 + bsig0(a) + maj(a, b, c);                                                    \
    }
    KPtr kp = (KPtr)&MIRSHA512_K(0);
    uint64_t kc[16], kn[16];
    MIRSHA512_K_FENCE(kp, a);
    MIRSHA512_UNROLL
    for (int i = 0; i < 16; i++) kc[i] = kp[i];
    MIRSHA512_UNROLL
    for (int j = 0; j < 80; j += 16) {
        if (j + 16 < 80) {
            MIRSHA512_K_FENCE(kp, a);
            MIRSHA512_UNROLL
            for (int i = 0; i < 16; i++) kn[i] = kp[j + 16 + i];
        }
        MIRSHA512_ROUND(a, b, c, d, e, f, g, h, j + 0);
        MIRSHA512_ROUND(h, a, b, c, d, e, f, g, j + 1);
        MIRSHA512_ROUND(g, h, a, b, c, d, e, f, j + 2);
        MIRSHA512_ROUND(f, g, h, a, b, c, d, e, j + 3);
        MIRSHA512_ROUND(e, f, g, h, a, b, c, d, j + 4);
        MIRSHA512_ROUND(d, e, f, g, h, a, b, c, j + 5);
        MIRSHA512_ROUND(c, d, e, f, g, h, a, b, j + 6);
        MIRSHA512_ROUND(b, c, d, e, f, g, h, a, j + 7);
        MIRSHA512_ROUND(a, b, c, d, e, f, g, h, j + 8);
        MIRSHA512_ROUND(h, a, b, c, d, e, f, g, j + 9);
        MIRSHA512_ROUND(g, h, a, b, c, d, e, f, j + 10);
        MIRSHA512_ROUND(f, g, h, a, b, c, d, e, j + 11);
        MIRSHA512_ROUND(e, f, g, h, a, b, c, d, j + 12);
        MIRSHA512_ROUND(d, e, f, g, h, a, b, c, j + 13);
        MIRSHA512_ROUND(c, d, e, f, g, h, a, b, j + 14);
        MIRSHA512_ROUND(b, c, d, e, f, g, h, a, j + 15);
        MIRSHA512_UNROLL
        for (int i = 0; i < 16; i++) kc[i] = kn[i];
    }
#undef MIRSHA512_ROUND
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// Number of 128-byte compressions for an L-byte message: (L + 16) / 128 + 1
// (0x80 and the 128-bit bit length need 17 bytes; the extra block comes when
// L % 128 >= 112), written so that no 32-bit L overflows.
MIRSHA512_HD uint32_t blocks_for_len(uint32_t L) { return (L >> 7) + 1u + ((L & 127u) >= 112u ? 1u : 0u); }

// FIPS 180-4 §5.1.2 padding of the block at message byte position p (a
// multiple of 128), in place.  bw[0..31] are the block's bytes as 32
// big-endian 32-bit words, read from wherever the message lies: whatever
// follows the message's last byte there (a neighbour's bytes, zeros past the
// arena) is masked off here, so it never reaches a digest.  `last`: the
// message's final block, which ends in the 128-bit big-endian bit length (its
// high 96 bits are zero for a 32-bit byte length).  Branch-free per word.
// Only for blocks that reach past the message's end, p + 128 > L (a block
// wholly inside the message needs nothing, and there L - p need not fit the
// signed difference below); every block of a message has p < L + 128.
MIRSHA512_HD void pad_block(uint32_t bw[32], uint32_t p, uint32_t L, bool last) {
    const int32_t left = (int32_t)(L - p);  // in (-128, 128)
    MIRSHA512_UNROLL
    for (int k = 0; k < 32; k++) {
        const int32_t t = left - 4 * k;                       // message bytes left at this word
        const uint32_t sh = ((uint32_t)t & 3u) << 3;          // only used when 0 <= t <= 3
        const uint32_t keep = ~(0xFFFFFFFFu >> sh);           // the t leading data bytes
        const uint32_t mark = 0x80000000u >> sh;              // the 0x80 byte right after them
        const uint32_t part = (bw[k] & keep) | mark;
        bw[k] = t >= 4 ? bw[k] : (t < 0 ? 0u : part);
    }
    if (last) {
        bw[30] = L >> 29;
        bw[31] = L << 3;
    }
}

// The 32 words of a block as the 16 words of the compression.
MIRSHA512_HD void join_words(const uint32_t bw[32], uint64_t w[16]) {
    MIRSHA512_UNROLL
    for (int i = 0; i < 16; i++) w[i] = ((uint64_t)bw[2 * i] << 32) | bw[2 * i + 1];
}

// One block of the message concat(c digest rows of 32 bytes): four rows fill a
// block.  rows[s] = the raw row (8 dwords as they lie in memory) of ordinal
// d0 + s, anything where d0 + s >= c; 0x80 goes where the list ends, and the
// final block (`last`) takes the bit length 256 c.  c % 4 == 0 (the empty list
// too) ends in a block that holds the marker and the length only; c % 4 == 3
// leaves bytes 96..127 for both, which is enough (marker at 96, length at 112).
MIRSHA512_HD void list_block(const uint32_t rows[4][8], uint32_t d0, uint32_t c, bool last, uint64_t w[16]) {
    MIRSHA512_UNROLL
    for (int s = 0; s < 4; s++) {
        const uint32_t d = d0 + (uint32_t)s;
    MIRSHA512_UNROLL
        for (int i = 0; i < 4; i++) {
            uint32_t hi = __builtin_bswap32(rows[s][2 * i]), lo = __builtin_bswap32(rows[s][2 * i + 1]);
            if (d >= c) {
                hi = (d == c && i == 0) ? 0x80000000u : 0u;
                lo = 0u;
            }
            w[4 * s + i] = ((uint64_t)hi << 32) | lo;
        }
    }
    if (last) {
        w[14] = 0u;
        w[15] = (uint64_t)c << 8;
    }
}

// The digest: the first 256 bits of the final state, big-endian, as the 8
// dwords a little-endian store writes.
MIRSHA512_HD void digest_words(const uint64_t st[8], uint32_t out[8]) {
    MIRSHA512_UNROLL
    for (int i = 0; i < 4; i++) {
        out[2 * i] = __builtin_bswap32((uint32_t)(st[i] >> 32));
        out[2 * i + 1] = __builtin_bswap32((uint32_t)st[i]);
    }
}

}  // namespace sha512
}  // namespace mirsha
