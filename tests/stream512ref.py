"""The reference the SHA-512/256 stream tests compare with
(tests/test_streams_hasher_host.py, tests/test_gpu_sha512_streams*.py), the
64-bit sibling of tests/streamref.py: hashlib hashers that also remember what
they were written, and the 204-byte state (Go 1.14 crypto/sha512 MarshalBinary
layout for New512_256) of such a hasher from a plain-Python SHA-512 compression
that is itself checked against hashlib.  Nothing here calls the code under
test."""
import hashlib
import struct

from mirbft_amd import STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE

CUTS = (STREAM_SUM_RESET, STREAM_RESET)
NAME = "sha512_256"
MAGIC = b"sha\x06"
STATE_BYTES = 204

K = [0x428a2f98d728ae22, 0x7137449123ef65cd, 0xb5c0fbcfec4d3b2f, 0xe9b5dba58189dbbc, 0x3956c25bf348b538,
     0x59f111f1b605d019, 0x923f82a4af194f9b, 0xab1c5ed5da6d8118, 0xd807aa98a3030242, 0x12835b0145706fbe,
     0x243185be4ee4b28c, 0x550c7dc3d5ffb4e2, 0x72be5d74f27b896f, 0x80deb1fe3b1696b1, 0x9bdc06a725c71235,
     0xc19bf174cf692694, 0xe49b69c19ef14ad2, 0xefbe4786384f25e3, 0x0fc19dc68b8cd5b5, 0x240ca1cc77ac9c65,
     0x2de92c6f592b0275, 0x4a7484aa6ea6e483, 0x5cb0a9dcbd41fbd4, 0x76f988da831153b5, 0x983e5152ee66dfab,
     0xa831c66d2db43210, 0xb00327c898fb213f, 0xbf597fc7beef0ee4, 0xc6e00bf33da88fc2, 0xd5a79147930aa725,
     0x06ca6351e003826f, 0x142929670a0e6e70, 0x27b70a8546d22ffc, 0x2e1b21385c26c926, 0x4d2c6dfc5ac42aed,
     0x53380d139d95b3df, 0x650a73548baf63de, 0x766a0abb3c77b2a8, 0x81c2c92e47edaee6, 0x92722c851482353b,
     0xa2bfe8a14cf10364, 0xa81a664bbc423001, 0xc24b8b70d0f89791, 0xc76c51a30654be30, 0xd192e819d6ef5218,
     0xd69906245565a910, 0xf40e35855771202a, 0x106aa07032bbd1b8, 0x19a4c116b8d2d0c8, 0x1e376c085141ab53,
     0x2748774cdf8eeb99, 0x34b0bcb5e19b48a8, 0x391c0cb3c5c95a63, 0x4ed8aa4ae3418acb, 0x5b9cca4f7763e373,
     0x682e6ff3d6b2b8a3, 0x748f82ee5defb2fc, 0x78a5636f43172f60, 0x84c87814a1f0ab72, 0x8cc702081a6439ec,
     0x90befffa23631e28, 0xa4506cebde82bde9, 0xbef9a3f7b2c67915, 0xc67178f2e372532b, 0xca273eceea26619c,
     0xd186b8c721c0c207, 0xeada7dd6cde0eb1e, 0xf57d4f7fee6ed178, 0x06f067aa72176fba, 0x0a637dc5a2c898a6,
     0x113f9804bef90dae, 0x1b710b35131c471b, 0x28db77f523047d84, 0x32caab7b40c72493, 0x3c9ebe0a15c9bebc,
     0x431d67c49c100d4c, 0x4cc5d4becb3e42b6, 0x597f299cfc657e2a, 0x5fcb6fab3ad6faec, 0x6c44198c4a475817]
H0 = (0x22312194fc2bf72c, 0x9f555fa3c84c64c2, 0x2393b86b6f53b151, 0x963877195940eabd, 0x96283ee2a88effe3,
      0xbe5e1e2553863992, 0x2b0199fc2c85b8aa, 0x0eb72ddc81c52ca2)  # FIPS 180-4 5.3.6.2
M64 = 0xFFFFFFFFFFFFFFFF


def rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def compress(h, block):
    """FIPS 180-4 6.4.2 in plain Python."""
    w = list(struct.unpack(">16Q", block))
    for j in range(16, 80):
        s0 = rotr(w[j - 15], 1) ^ rotr(w[j - 15], 8) ^ (w[j - 15] >> 7)
        s1 = rotr(w[j - 2], 19) ^ rotr(w[j - 2], 61) ^ (w[j - 2] >> 6)
        w.append((w[j - 16] + s0 + w[j - 7] + s1) & M64)
    a, b, c, d, e, f, g, hh = h
    for j in range(80):
        t1 = (hh + (rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)) + ((e & f) ^ (~e & g & M64)) + K[j] + w[j]) & M64
        t2 = ((rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c))) & M64
        a, b, c, d, e, f, g, hh = (t1 + t2) & M64, a, b, c, (d + t1) & M64, e, f, g
    return [(x + y) & M64 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


def finish(h, tail: bytes, total: int) -> bytes:
    """The digest of a hasher with midstate h, `tail` buffered and `total`
    bytes written: the padding with the 128-bit bit length, the last blocks."""
    tail = tail + b"\x80"
    tail += bytes(-(len(tail) + 16) % 128) + (8 * total).to_bytes(16, "big")
    h = list(h)
    for i in range(0, len(tail), 128):
        h = compress(h, tail[i:i + 128])
    return struct.pack(">8Q", *h)[:32]


def sha512_256_by_hand(data: bytes) -> bytes:
    h = list(H0)
    whole = len(data) // 128 * 128
    for i in range(0, whole, 128):
        h = compress(h, data[i:i + 128])
    return finish(h, data[whole:], len(data))


def marshal(h, tail: bytes, total: int) -> bytes:
    """The 204-byte state: the magic, h as big-endian u64, the buffered bytes
    zero-padded to 128, the total length as big-endian u64."""
    return MAGIC + struct.pack(">8Q", *h) + tail.ljust(128, b"\0") + struct.pack(">Q", total)


def marshal_of(data: bytes) -> bytes:
    """The state of a hasher that was written `data`."""
    h = list(H0)
    whole = len(data) // 128 * 128
    for i in range(0, whole, 128):
        h = compress(h, data[i:i + 128])
    return marshal(h, data[whole:], len(data))


def continue_from(h, tail: bytes, total: int, more: bytes) -> bytes:
    """The digest after writing `more` to a hasher in the state (h, tail, total),
    whatever was written before (a hand-built state with a huge length)."""
    buf = tail + more
    h = list(h)
    whole = len(buf) // 128 * 128
    for i in range(0, whole, 128):
        h = compress(h, buf[i:i + 128])
    return finish(h, buf[whole:], total + len(more))


class Walker:
    """A hashlib hasher that also remembers what it was written since its last reset."""

    def __init__(self, written=b"", name=NAME):
        self.name = name
        self.h, self.written = hashlib.new(name, written), written

    def run(self, kind, data=b""):
        """One op; returns the value of a sum, else None."""
        if kind == STREAM_WRITE:
            self.h.update(data)
            self.written += data
            return None
        value = self.h.digest() if kind in (STREAM_SUM, STREAM_SUM_RESET) else None
        if kind in CUTS:
            self.h, self.written = hashlib.new(self.name), b""
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
