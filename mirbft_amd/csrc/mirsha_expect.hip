// mirsha_expect.hip — the select kernels of the mixed hash-and-verify ring
// submissions (mirsha_submit_*_expect and, deduplicated,
// mirsha_submit_slices_expect_dedup; mirsha_async.hip).  A translation unit
// of its own: the hashing kernels' sources and code object are untouched.
#include "mirsha_ctx.h"

namespace mirsha {

// A Ready() cycle whose requests may or may not carry the digest their origin
// expects: has[] marks the requests that do, row base[w] + popcount(has[w]
// below the lane) of `want` is such a request's expectation
// (mirsha_expect_plan).  One lane per request, one wave per bitmap word, as
// verify_digests_kernel.  A lane whose bit is set compares its digest with its
// expectation row (set lanes map to consecutive rows); the wave's ballot is
// the mismatch word.  A request without an expectation and every mismatch
// stores its 32-byte digest row to row i of `out` (host-visible page-locked
// memory: only these rows cross PCIe); a match stores nothing.  Lane 0 stores
// the mismatch word and a wave with mismatches adds their number to *count
// with one atomic.  Waves that start at or beyond n do nothing.
__global__ __launch_bounds__(kBlockThreads) void expect_select_kernel(const uint4* __restrict__ dig,
                                                                      const uint4* __restrict__ want,
                                                                      const unsigned long long* __restrict__ has,
                                                                      const uint32_t* __restrict__ base, uint32_t n,
                                                                      uint4* __restrict__ out,
                                                                      unsigned long long* __restrict__ bits,
                                                                      uint32_t* __restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (i - lane >= n) return;  // the whole wave: no word of the bitmap
    const uint64_t w = i >> 6;
    const unsigned long long h = has[w];
    const bool in = i < n;
    const bool mine = in && ((h >> lane) & 1ull) != 0ull;
    uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0;
    if (in) {
        a0 = dig[2u * i];
        a1 = dig[2u * i + 1u];
    }
    bool differs = false;
    if (mine) {
        const uint64_t k = (uint64_t)base[w] + (uint32_t)__popcll(h & ((1ull << lane) - 1ull));
        const uint4 b0 = want[2u * k], b1 = want[2u * k + 1u];
        differs = (((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w)) |
                   ((a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w))) != 0u;
    }
    const unsigned long long mis = __ballot(differs);
    if (in && (!mine || differs)) {  // keep = ~has | mis, below n
        out[2u * i] = a0;
        out[2u * i + 1u] = a1;
    }
    if (lane == 0u) {
        bits[w] = mis;
        if (mis) atomicAdd(count, (uint32_t)__popcll(mis));
    }
}

hipError_t launch_expect_select(const uint8_t* digests, const uint8_t* expected, const uint64_t* has,
                                const uint32_t* base, uint32_t n, uint8_t* out, uint64_t* bits, uint32_t* count,
                                hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + kBlockThreads - 1u) / kBlockThreads);
    const uint4* d = reinterpret_cast<const uint4*>(digests);
    const uint4* e = reinterpret_cast<const uint4*>(expected);
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(has);
    uint4* o = reinterpret_cast<uint4*>(out);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(bits);
    launch_k(expect_select_kernel, grid, kBlockThreads, 0, s, d, e, h, base, n, o, b, count);
    return hipGetLastError();
}

// expect_select_kernel for a deduplicated cycle (mirsha_submit_slices_expect_dedup):
// only one request per distinct content was hashed, so lane i reads its digest
// from row row_of[i] of the representatives' digests (mirsha_dedup_rows) and
// not from row i.  Those rows lie in two arrays, one per hashing launch of the
// submission: rows [0, m0) in dig0, rows [m0, m) in dig1 (never read when the
// submission had one launch: then m0 = m).  Everything else is
// expect_select_kernel: the lane's own expectation row, the wave's ballot, the
// kept rows stored to row i of `out`, so a duplicate's verdict and row are
// those of its own bytes' digest against its own expectation.
__global__ __launch_bounds__(kBlockThreads) void expect_select_gather_kernel(
    const uint4* __restrict__ dig0, const uint4* __restrict__ dig1, uint32_t m0, const uint32_t* __restrict__ row_of,
    const uint4* __restrict__ want, const unsigned long long* __restrict__ has, const uint32_t* __restrict__ base,
    uint32_t n, uint4* __restrict__ out, unsigned long long* __restrict__ bits, uint32_t* __restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (i - lane >= n) return;  // the whole wave: no word of the bitmap
    const uint64_t w = i >> 6;
    const unsigned long long h = has[w];
    const bool in = i < n;
    const bool mine = in && ((h >> lane) & 1ull) != 0ull;
    uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0;
    if (in) {
        const uint32_t r = row_of[i];
        const uint4* src = r < m0 ? dig0 + 2ull * r : dig1 + 2ull * (r - m0);
        a0 = src[0];
        a1 = src[1];
    }
    bool differs = false;
    if (mine) {
        const uint64_t k = (uint64_t)base[w] + (uint32_t)__popcll(h & ((1ull << lane) - 1ull));
        const uint4 b0 = want[2u * k], b1 = want[2u * k + 1u];
        differs = (((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w)) |
                   ((a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w))) != 0u;
    }
    const unsigned long long mis = __ballot(differs);
    if (in && (!mine || differs)) {  // keep = ~has | mis, below n
        out[2u * i] = a0;
        out[2u * i + 1u] = a1;
    }
    if (lane == 0u) {
        bits[w] = mis;
        if (mis) atomicAdd(count, (uint32_t)__popcll(mis));
    }
}

hipError_t launch_expect_select_gather(const uint8_t* digests0, const uint8_t* digests1, uint32_t m0,
                                       const uint32_t* row_of, const uint8_t* expected, const uint64_t* has,
                                       const uint32_t* base, uint32_t n, uint8_t* out, uint64_t* bits,
                                       uint32_t* count, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + kBlockThreads - 1u) / kBlockThreads);
    const uint4* d0 = reinterpret_cast<const uint4*>(digests0);
    const uint4* d1 = reinterpret_cast<const uint4*>(digests1);
    const uint4* e = reinterpret_cast<const uint4*>(expected);
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(has);
    uint4* o = reinterpret_cast<uint4*>(out);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(bits);
    launch_k(expect_select_gather_kernel, grid, kBlockThreads, 0, s, d0, d1, m0, row_of, e, h, base, n, o, b, count);
    return hipGetLastError();
}

}  // namespace mirsha
