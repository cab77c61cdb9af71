// mirsha_order.hip — the kernels of the device-built bucket order
// (mirsha_order.h: mirsha_bucket_order_device and the ring's device order
// mode).  A translation unit of its own: the hashing kernels' sources and
// code object are untouched.
#include "mirsha_device.h"
#include "mirsha_order.h"

namespace mirsha {

namespace {
constexpr uint32_t kOrderWave = 64;  // one wave per workgroup: its LDS histogram is its own

// blocks(L) = ceil((L + 9) / 64) without leaving 32 bits (host_blocks), then
// the bin: longest first, lengths outside the bounds at the nearest one.
__device__ __forceinline__ uint32_t order_bin(uint32_t L, uint32_t bmax, uint32_t bins) {
    const uint32_t b = (L >> 6) + (((L & 63u) + 72u) >> 6);
    return b >= bmax ? 0u : min(bmax - b, bins - 1u);
}
}  // namespace

// Wave c counts its chunk [c * chunk, min(n, (c + 1) * chunk)), 64 indices a
// step, into a histogram of `bins` words in its own LDS, then stores it
// bin-major: counts[bin * n_chunks + c].
__global__ __launch_bounds__(kOrderWave) void order_count_kernel(const uint32_t* __restrict__ len, uint32_t n,
                                                                 uint32_t bmax, uint32_t bins, uint32_t chunk,
                                                                 uint32_t n_chunks, uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t order_hist[];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    for (uint32_t b = lane; b < bins; b += kOrderWave) order_hist[b] = 0u;
    __syncthreads();
    const uint64_t first = (uint64_t)c * chunk;
    const uint64_t end = min((uint64_t)n, first + chunk);
    for (uint64_t i0 = first; i0 < end; i0 += kOrderWave) {
        const uint64_t i = i0 + lane;
        if (i < end) atomicAdd(&order_hist[order_bin(len[i], bmax, bins)], 1u);
    }
    __syncthreads();
    for (uint32_t b = lane; b < bins; b += kOrderWave) counts[(uint64_t)b * n_chunks + c] = order_hist[b];
}

// The same chunking; the wave's LDS holds the next free position of each of
// its (bin, chunk) cells, first the scanned bases.  Per step the lanes that
// share a bin form a group, found one group a turn: the first remaining lane's
// bin is broadcast, a ballot marks its group, a group lane's rank is the bin's
// position plus the group lanes below it, and the first lane moves the position
// on by the group's size.  Every turn retires at least that first lane, so a
// step ends after at most 64 turns.  The position's load feeds its store, and
// both are issued for the whole wave, so no lane reads a moved position.
__global__ __launch_bounds__(kOrderWave) void order_scatter_kernel(const uint32_t* __restrict__ len, uint32_t n,
                                                                   uint32_t bmax, uint32_t bins, uint32_t chunk,
                                                                   uint32_t n_chunks,
                                                                   const uint32_t* __restrict__ base,
                                                                   uint32_t* __restrict__ order) {
    extern __shared__ uint32_t order_pos[];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    for (uint32_t b = lane; b < bins; b += kOrderWave) order_pos[b] = base[(uint64_t)b * n_chunks + c];
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint64_t first = (uint64_t)c * chunk;
    const uint64_t end = min((uint64_t)n, first + chunk);
    for (uint64_t i0 = first; i0 < end; i0 += kOrderWave) {
        const uint64_t i = i0 + lane;
        const bool in = i < end;
        const uint32_t bin = in ? order_bin(len[i], bmax, bins) : 0xFFFFFFFFu;
        uint32_t rank = 0u;
        unsigned long long rem = __ballot(in);
        while (rem) {
            const uint32_t lead = (uint32_t)__ffsll((long long)rem) - 1u;
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)lead);  // < bins: lane `lead` is in
            const unsigned long long grp = __ballot(bin == b0);
            const uint32_t p = order_pos[b0];
            if (bin == b0) rank = p + (uint32_t)__popcll(grp & below);
            if (lane == lead) order_pos[b0] = p + (uint32_t)__popcll(grp);
            rem &= ~grp;
        }
        // rank < n whenever the bases are the scan of this len[]'s counts; the
        // guard keeps a len[] changed between the launches from storing outside order[]
        if (in && rank < n) order[rank] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kOrderWave) void order_iota_kernel(uint32_t* __restrict__ order, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kOrderWave + threadIdx.x;
    if (i < n) order[i] = (uint32_t)i;
}

hipError_t launch_order_count(const uint32_t* len, uint32_t n, uint32_t bmax, uint32_t bins, uint32_t chunk,
                              uint32_t n_chunks, uint32_t* counts, hipStream_t s) {
    if (n_chunks == 0) return hipSuccess;
    launch_k(order_count_kernel, n_chunks, kOrderWave, 4u * bins, s, len, n, bmax, bins, chunk, n_chunks, counts);
    return hipGetLastError();
}

hipError_t launch_order_scatter(const uint32_t* len, uint32_t n, uint32_t bmax, uint32_t bins, uint32_t chunk,
                                uint32_t n_chunks, const uint32_t* base, uint32_t* order, hipStream_t s) {
    if (n_chunks == 0) return hipSuccess;
    launch_k(order_scatter_kernel, n_chunks, kOrderWave, 4u * bins, s, len, n, bmax, bins, chunk, n_chunks, base,
             order);
    return hipGetLastError();
}

hipError_t launch_order_iota(uint32_t* order, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + kOrderWave - 1u) / kOrderWave);
    launch_k(order_iota_kernel, grid, kOrderWave, 0, s, order, n);
    return hipGetLastError();
}

}  // namespace mirsha
