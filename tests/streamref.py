"""The reference the streams' ring tests compare with (tests/test_streams_ring_host.py,
tests/test_gpu_streams_ring.py): hashlib hashers that also remember what they
were written, and the 108-byte state (Go 1.14 crypto/sha256 MarshalBinary
layout) of such a hasher from a plain-Python compression that is itself
checked against hashlib.  Nothing here calls the code under test."""
import hashlib
import struct

from mirbft_amd import STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE

CUTS = (STREAM_SUM_RESET, STREAM_RESET)

K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
     0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
     0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
     0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
     0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
     0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
     0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
     0xc67178f2]
H0 = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
M32 = 0xFFFFFFFF


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(h, block):
    """FIPS 180-4 6.2.2 in plain Python."""
    w = list(struct.unpack(">16I", block))
    for j in range(16, 64):
        s0 = rotr(w[j - 15], 7) ^ rotr(w[j - 15], 18) ^ (w[j - 15] >> 3)
        s1 = rotr(w[j - 2], 17) ^ rotr(w[j - 2], 19) ^ (w[j - 2] >> 10)
        w.append((w[j - 16] + s0 + w[j - 7] + s1) & M32)
    a, b, c, d, e, f, g, hh = h
    for j in range(64):
        t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + K[j] + w[j]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        a, b, c, d, e, f, g, hh = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
    return [(x + y) & M32 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


def sha256_by_hand(data: bytes) -> bytes:
    tail = data + b"\x80"
    tail += bytes(-(len(tail) + 8) % 64) + struct.pack(">Q", 8 * len(data))
    h = list(H0)
    for i in range(0, len(tail), 64):
        h = compress(h, tail[i:i + 64])
    return struct.pack(">8I", *h)


def marshal_of(data: bytes) -> bytes:
    """The 108-byte state of a hasher that was written `data`: the magic, the
    midstate behind its whole blocks, the rest zero-padded to 64, the length."""
    h = list(H0)
    whole = len(data) // 64 * 64
    for i in range(0, whole, 64):
        h = compress(h, data[i:i + 64])
    return b"sha\x03" + struct.pack(">8I", *h) + data[whole:].ljust(64, b"\0") + struct.pack(">Q", len(data))


class Walker:
    """A hashlib hasher that also remembers what it was written since its last reset."""

    def __init__(self, written=b""):
        self.h, self.written = hashlib.sha256(written), written

    def run(self, kind, data=b""):
        """One op; returns the value of a sum, else None."""
        if kind == STREAM_WRITE:
            self.h.update(data)
            self.written += data
            return None
        value = self.h.digest() if kind in (STREAM_SUM, STREAM_SUM_RESET) else None
        if kind in CUTS:
            self.h, self.written = hashlib.sha256(), b""
        return value


def run_ref(ref, arena, ops):
    """The programme on the Walkers ref[stream], in op order; the sums' values."""
    out = []
    for op in ops:
        s, kind = int(op[0]), int(op[1])
        off, ln = (int(op[2]), int(op[3])) if kind == STREAM_WRITE else (0, 0)
        v = ref[s].run(kind, bytes(arena[off:off + ln]))
        if v is not None:
            out.append(v)
    return out
