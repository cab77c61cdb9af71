// mirsha_sha512.hip — the two kernels of the second hasher, SHA-512/256
// (sha512.New512_256 as a Processor's `Hasher`, processor.go:21,58):
//
//   sha512_msgs_kernel   one lane per message of an arena, any byte alignment
//   sha512_lists_kernel  one lane per digest list (four 32-byte rows a block)
//
// A translation unit and code object of its own: the SHA-256 kernels' sources
// are untouched.  Everything that decides bytes is sha512_device.h (proved on
// the CPU); the loaders and the per-lane bodies are sha512_lanes.h, which the
// plans' unit (mirsha_sha512_plan.hip) shares.  Both kernels use no LDS, no
// atomics, no waiting; lanes depend on each other only through the block
// loop's ballot.
#include "mirsha_sha512.h"

#include "sha512_lanes.h"

namespace mirsha {

// One lane per message of the arena (sha512_msg_lane, sha512_lanes.h).
__global__ __launch_bounds__(kSha512Threads) void sha512_msgs_kernel(
    const uint8_t* __restrict__ arena, uint64_t arena_len, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, const uint32_t* __restrict__ order, uint32_t n, uint8_t* __restrict__ out) {
    sha512_msg_lane(arena, arena_len, off, len, order, n, out, blockIdx.x * kSha512Threads + threadIdx.x);
}

// Dependent pass: one lane per digest list, nulls skipped in the walk
// (sha512_list_lane, sha512_lanes.h).
__global__ __launch_bounds__(kSha512Threads) void sha512_lists_kernel(
    const uint8_t* __restrict__ digests, uint32_t n_digests, const uint32_t* __restrict__ idx, uint32_t n_entries,
    const uint32_t* __restrict__ first, uint32_t n_lists, uint8_t* __restrict__ out) {
    sha512_list_lane(digests, n_digests, idx, n_entries, first, n_lists, out, blockIdx.x * kSha512Threads + threadIdx.x);
}

hipError_t launch_sha512_msgs(const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                              const uint32_t* order, uint32_t n, uint8_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (arena_len > kMaxBufferArena || n >= kMaxBufferMsgs) return hipErrorInvalidValue;
    const uint32_t grid = (n + kSha512Threads - 1u) / kSha512Threads;
    launch_k(sha512_msgs_kernel, grid, kSha512Threads, 0, s, arena, arena_len, off, len, order, n, out);
    return hipGetLastError();
}

hipError_t launch_sha512_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* idx, uint32_t n_entries,
                               const uint32_t* first, uint32_t n_lists, uint32_t* /*scratch*/, uint8_t* out,
                               hipStream_t s) {
    if (n_lists == 0) return hipSuccess;
    const uint32_t grid = (n_lists + kSha512Threads - 1u) / kSha512Threads;
    launch_k(sha512_lists_kernel, grid, kSha512Threads, 0, s, digests, n_digests, idx, n_entries, first, n_lists, out);
    return hipGetLastError();
}

}  // namespace mirsha
