// mirsha_sha512.h — launchers of the SHA-512/256 kernels (mirsha_sha512.hip):
// the request and the list kernel of a context whose hasher is
// MIRSHA_HASHER_SHA512_256: the one-lane kernels, which the routed launchers of
// mirsha_sha512_pair.h (what hasher_launch_msgs / _lists queue, mirsha_ctx.h)
// take for every launch that is not small.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// launch_msgs' arguments without `variant`: one form serves every launch
// size.  The arena goes through one 32-bit buffer descriptor and the digests
// through 32-bit row offsets: arena_len > kMaxBufferArena or n >=
// kMaxBufferMsgs is hipErrorInvalidValue (there is no 64-bit-addressed form).
hipError_t launch_sha512_msgs(const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                              const uint32_t* order, uint32_t n, uint8_t* out, hipStream_t s);
// launch_lists' arguments; `scratch` is unused (nulls are skipped in the walk).
hipError_t launch_sha512_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* idx, uint32_t n_entries,
                               const uint32_t* first, uint32_t n_lists, uint32_t* scratch, uint8_t* out,
                               hipStream_t s);

}  // namespace mirsha
