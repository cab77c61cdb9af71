// mirsha_sha512_plan.h — launchers of the device plans' kernels under the
// second hasher, SHA-512/256 (mirsha_sha512_plan.hip): the dependent pass of a
// plan and the overlapped cycle (pipeline_run, mirsha_pipeline_overlap_device;
// mirsha_plan.hip).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// A plan's compacted lists (no MIRSHA_NULL_INDEX entry), one lane per list.
// uniform = B > 0: identity lists of B entries (launch_chain's contract);
// cidx / cfirst unread.  Index reads are range-checked against n_entries, row
// reads against n_digests.
hipError_t launch_sha512_plan_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* cidx,
                                    uint32_t n_entries, const uint32_t* cfirst, uint32_t n_lists, uint32_t uniform,
                                    uint8_t* out, hipStream_t s);

// An overlapped cycle in one launch: list_blocks workgroups walk the plan's
// lists over the PREVIOUS cycle's request digests (complete: nothing waits),
// then tile_blocks workgroups hash this cycle's requests, lane slot = message
// order[slot].  The limits of launch_sha512_msgs hold for arena_len and n_req.
struct Sha512OverlapArgs {
    const uint8_t* arena;
    uint64_t arena_len;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* order;  // NULL = identity
    uint32_t n_req;         // this cycle's requests (0: chains only)
    uint8_t* req_out;
    const uint8_t* prev_digests;  // previous cycle's request digests
    uint32_t n_req_prev;
    const uint32_t* cidx;
    uint32_t n_entries;
    const uint32_t* cfirst;
    uint32_t n_lists;  // 0: no chains this launch (the first cycle)
    uint32_t uniform;
    uint8_t* list_out;
    uint32_t list_blocks;  // set by the launcher: ceil(n_lists / 256), first in the grid
};
hipError_t launch_sha512_overlap(const Sha512OverlapArgs& a, hipStream_t s);

}  // namespace mirsha
