// mirsha_sha512_plan.hip — the kernels of the device plans under the second
// hasher, SHA-512/256 (mirsha_pipeline_create_hasher):
//
//   sha512_plan_lists_kernel<kUniform>  the dependent pass of a plan: one lane
//                                       per compacted list, indices loaded
//                                       (<false>) or computed (<true>)
//   sha512_overlap_kernel               an overlapped cycle in one launch: the
//                                       previous cycle's lists, then this
//                                       cycle's requests
//
// A translation unit and code object of its own: mirsha_sha512.hip keeps its
// two kernels, the SHA-256 kernels' sources are untouched.  The per-lane bodies
// are sha512_lanes.h.  No LDS, no atomics, no waiting, no communication between
// workgroups; every register index is static.
#include "mirsha_sha512_plan.h"

#include "sha512_lanes.h"

namespace mirsha {

template <bool kUniform>
__global__ __launch_bounds__(kSha512Threads) void sha512_plan_lists_kernel(
    const uint8_t* __restrict__ digests, uint32_t n_digests, const uint32_t* __restrict__ cidx, uint32_t n_entries,
    const uint32_t* __restrict__ cfirst, uint32_t n_lists, uint32_t uniform, uint8_t* __restrict__ out) {
    sha512_plan_list_lane<kUniform>(digests, n_digests, cidx, n_entries, cfirst, n_lists, uniform, out,
                                    blockIdx.x * kSha512Threads + threadIdx.x);
}

// Grid: list_blocks + tile_blocks workgroups.  The list blocks come first, so
// their chains of c / 4 + 1 dependent compressions start with the launch and
// do not form its tail; they read the previous cycle's digests, which are
// complete, so no block waits on another.  The role is decided by blockIdx.x:
// uniform over a workgroup.  A role whose count is 0 has no blocks (the first
// cycle: tiles only; the flush: chains only).
__global__ __launch_bounds__(kSha512Threads) void sha512_overlap_kernel(Sha512OverlapArgs a) {
    if (blockIdx.x < a.list_blocks) {
        const uint32_t k = blockIdx.x * kSha512Threads + threadIdx.x;
        if (a.n_lists == 0u) return;
        if (a.uniform)
            sha512_plan_list_lane<true>(a.prev_digests, a.n_req_prev, a.cidx, a.n_entries, a.cfirst, a.n_lists,
                                        a.uniform, a.list_out, k);
        else
            sha512_plan_list_lane<false>(a.prev_digests, a.n_req_prev, a.cidx, a.n_entries, a.cfirst, a.n_lists, 0u,
                                         a.list_out, k);
        return;
    }
    if (a.n_req == 0u) return;
    sha512_msg_lane(a.arena, a.arena_len, a.off, a.len, a.order, a.n_req, a.req_out,
                    (blockIdx.x - a.list_blocks) * kSha512Threads + threadIdx.x);
}

hipError_t launch_sha512_plan_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* cidx,
                                    uint32_t n_entries, const uint32_t* cfirst, uint32_t n_lists, uint32_t uniform,
                                    uint8_t* out, hipStream_t s) {
    if (n_lists == 0) return hipSuccess;
    const uint32_t grid = (n_lists + kSha512Threads - 1u) / kSha512Threads;
    if (uniform)
        launch_k(sha512_plan_lists_kernel<true>, grid, kSha512Threads, 0, s, digests, n_digests, cidx, n_entries,
                 cfirst, n_lists, uniform, out);
    else
        launch_k(sha512_plan_lists_kernel<false>, grid, kSha512Threads, 0, s, digests, n_digests, cidx, n_entries,
                 cfirst, n_lists, 0u, out);
    return hipGetLastError();
}

hipError_t launch_sha512_overlap(const Sha512OverlapArgs& args, hipStream_t s) {
    if (args.arena_len > kMaxBufferArena || args.n_req >= kMaxBufferMsgs) return hipErrorInvalidValue;
    Sha512OverlapArgs a = args;
    a.list_blocks = (a.n_lists + kSha512Threads - 1u) / kSha512Threads;
    const uint32_t tile_blocks = (a.n_req + kSha512Threads - 1u) / kSha512Threads;
    if (a.list_blocks + tile_blocks == 0) return hipSuccess;
    launch_k(sha512_overlap_kernel, a.list_blocks + tile_blocks, kSha512Threads, 0, s, a);
    return hipGetLastError();
}

}  // namespace mirsha
