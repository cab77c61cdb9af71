// mirsha_sha512_streams.h — launchers of the streaming hash states of the
// second hasher, SHA-512/256 (mirsha_sha512_streams.hip): the SHA-512/256 row
// of stream_kernels (mirsha_streams.h), whose members' contracts they follow.
// Not part of the C-ABI.  The step itself is sha512_stream.h.
//
// State of stream s, device-resident and kept across calls: row s of
// kSha512StreamStateBytes bytes of one array (a whole number of 16-byte
// accesses, one address per lane for the load and the store):
//   [0, 64)     h[8], u64
//   [64, 192)   the unfinished block as 32 big-endian u32 words; only its
//               first count % 128 bytes mean anything
//   [192, 200)  the total bytes written, u64
//   [200, 208)  unused
//
// The window, in the arena's 32-bit offsets (arena_words, shift, span as in
// mirsha_streams.h; span <= MIRSHA_MAX_DEVICE_ARENA_BYTES + 6 rounded down to
// 4 = 0xFFFFFF04):
//   begin  a write at arena offset 0 that arrives at fill 127 has its window
//          at a = shift - 127 >= -127; rounded down to 4, the first word lies
//          at -128 = 0xFFFFFF80 (mod 2^32) or above: at or above every span,
//          so it is not loaded (its bytes are the block's own, never under the
//          merge mask), and the offsets wrap to 0 exactly where the arena
//          begins.  (Counted from the arena's own first byte, which lies at
//          `shift`, that is up to 127 + 3 bytes before the arena.)
//   end    a window begins at or before the write position (a <= span), and
//          its 33 words end at most 128 + 4 bytes behind it: the largest
//          offset formed is below 0xFFFFFF04 + 132 < 2^32, so nothing wraps
//          back into the arena; words at or above span are not loaded, and
//          words below it lie inside the allocation, which the host forms end
//          with kArenaSlack = 256 >= 132 bytes of slack (mirsha_ctx.h) and the
//          device forms with the arena's own last aligned word.
//   dead   ld_u32's dead offset 0xFFFFFFF0 is above every span as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

constexpr uint32_t kSha512StreamStateBytes = 208;

// Hasher() of a SHA-512/256 stream: one device row (host code).
void sha512_stream_row0(uint8_t* row);

// As launch_streams / launch_streams_seg (mirsha_streams.h), rows of
// kSha512StreamStateBytes.
hipError_t launch_sha512_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                                 const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s);
hipError_t launch_sha512_streams_seg(const uint32_t* arena_words, uint32_t shift, uint32_t span,
                                     const uint32_t* seg_stream, const uint32_t* sfirst, const uint32_t* seg_flags,
                                     const uint32_t* ent, uint32_t n_seg, const uint8_t* state_in, uint8_t* state,
                                     uint8_t* out, uint32_t prio, hipStream_t s);

}  // namespace mirsha
