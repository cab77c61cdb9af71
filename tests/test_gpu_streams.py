"""Streaming hash states on the device (mirsha_streams_*: HashStreams, its
hash.Hash form and StreamLog): Write / Sum / Reset over any bytes, bit-exact
against hashlib.  Every case is one or a few launches over a few KB."""
import hashlib
import struct

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, Actions, Checkpoint, CheckpointChains,
                        Commit, CommitBatch, DeviceLog, GpuHash, HashStreams, MirshaError, Processor, StreamLog, _lib)
from mirbft_amd.engine import KERNEL_STREAMS
from mirbft_amd.hashdata import uint64_to_bytes

pytestmark = pytest.mark.gpu

EMPTY = hashlib.sha256(b"").digest()
W, S, SR, R = STREAM_WRITE, STREAM_SUM, STREAM_SUM_RESET, STREAM_RESET

# ---- fill x length: one stream per (b, L), Write(b bytes), Write(L bytes), Sum ----------
FILLS, LENGTHS = 64, 131
POOL = np.random.default_rng(0x57).integers(0, 256, FILLS * LENGTHS + 300, dtype=np.uint8).tobytes()


def fl_parts(s):
    """Stream s = (b, L): its two writes' bytes (content differs per stream)."""
    b, L = divmod(s, LENGTHS)
    return POOL[s:s + b], POOL[s + 77:s + 77 + L]


_fl_want = []


def fl_want():
    """The hashlib digests of the fill x length streams: computed once, shared."""
    if not _fl_want:
        _fl_want.append([hashlib.sha256(b"".join(fl_parts(s))).digest() for s in range(FILLS * LENGTHS)])
    return _fl_want[0]


def fl_programme(align=None):
    """(ops, arena): with `align` the L-byte range of every stream starts at an
    arena offset = align (mod 16), else the ranges lie back to back."""
    n = FILLS * LENGTHS
    arena = bytearray()
    off = np.zeros((n, 3), dtype=np.uint64)
    ln = np.zeros((n, 3), dtype=np.uint32)
    for s in range(n):
        head, body = fl_parts(s)
        off[s, 0], ln[s, 0] = len(arena), len(head)
        arena += head
        if align is not None:
            arena += bytes((align - len(arena)) % 16)
        off[s, 1], ln[s, 1] = len(arena), len(body)
        arena += body
    stream = np.repeat(np.arange(n, dtype=np.uint32), 3)
    kind = np.tile(np.asarray([W, W, S], dtype=np.uint32), n)
    return (stream, kind, off.reshape(-1), ln.reshape(-1)), bytes(arena)


def digests(rows):
    return [r.tobytes() for r in rows]


def test_fill_times_length_in_one_run(engine):
    hs = HashStreams(engine, FILLS * LENGTHS)
    ops, arena = fl_programme()
    assert digests(hs.run(ops, arena)) == fl_want()
    hs.close()


@pytest.mark.parametrize("align", range(16))
def test_fill_times_length_at_every_arena_alignment(engine, align):
    """The device form reads the arena where it lies, so the L-byte range really
    sits at that alignment (the host form packs the written bytes)."""
    import torch

    hs = HashStreams(engine, FILLS * LENGTHS)
    ops, arena = fl_programme(align)
    assert all(int(o) % 16 == align for o in ops[2][1::3])
    t = torch.frombuffer(bytearray(arena), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert digests(hs.run_device(ops, t.data_ptr(), len(arena))) == fl_want()
    hs.close()


def test_fill_times_length_through_run_device(engine):
    """The dense layout from a torch tensor, at an odd device address too."""
    import torch

    ops, arena = fl_programme()
    for lead in (0, 1):
        hs = HashStreams(engine, FILLS * LENGTHS)
        t = torch.frombuffer(bytearray(bytes(lead) + arena), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert digests(hs.run_device(ops, t.data_ptr() + lead, len(arena))) == fl_want(), lead
        hs.close()


# ---- arena edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_form", [False, True])
def test_write_range_at_arena_offset_0_arriving_at_a_fill(engine, device_form):
    """The stream-aligned window of such a write begins before the arena."""
    import torch

    rng = np.random.default_rng(21)
    fills, lens = (1, 3, 17, 63), (1, 2, 61, 64, 100)
    hs = HashStreams(engine, len(fills) * len(lens))
    for k, f in enumerate(fills):
        for j, L in enumerate(lens):
            s = k * len(lens) + j
            head, body = rng.bytes(f), rng.bytes(L)
            hs.run([(s, W, 0, f)], head)
            ops = [(s, W, 0, L), (s, S)]
            if device_form:
                t = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                got = hs.run_device(ops, t.data_ptr(), L)
            else:
                got = hs.run(ops, body)
            assert got[0].tobytes() == hashlib.sha256(head + body).digest(), (f, L)
    hs.close()


@pytest.mark.parametrize("device_form", [False, True])
def test_write_ranges_ending_at_the_arenas_last_byte(engine, device_form):
    import torch

    rng = np.random.default_rng(22)
    A = 203  # not a multiple of 4
    arena = rng.bytes(A)
    hs = HashStreams(engine, 81)
    ops = [(80, W, 0, 1)]  # the host form's packed bytes: 1 + (1 + ... + 80) = 3241, not a multiple of 4 either
    for L in range(1, 81):
        ops += [(L - 1, W, A - L, L), (L - 1, S)]
    if device_form:
        t = torch.frombuffer(bytearray(arena), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        got = hs.run_device(ops, t.data_ptr(), A)
    else:
        got = hs.run(ops, arena)
    assert digests(got) == [hashlib.sha256(arena[A - L:]).digest() for L in range(1, 81)]
    hs.close()


# ---- padding edges -------------------------------------------------------------------------
def test_padding_edges_and_sum_leaves_the_state(engine):
    rng = np.random.default_rng(23)
    totals = (0, 55, 56, 63, 64, 119, 120, 128)
    data = rng.bytes(300)
    hs = HashStreams(engine, len(totals) + 1)
    ops = []
    for s, n in enumerate(totals):
        ops += [(s, W, 7, n), (s, S)]
    assert digests(hs.run(ops, data)) == [hashlib.sha256(data[7:7 + n]).digest() for n in totals]
    # write, sum, write, sum: the two prefixes' digests; again over two calls, and a repeated Sum
    s = len(totals)
    got = hs.run([(s, W, 0, 60), (s, S), (s, W, 60, 70), (s, S), (s, S)], data)
    assert digests(got) == [hashlib.sha256(data[:60]).digest()] + [hashlib.sha256(data[:130]).digest()] * 2
    got = hs.run([(s, S), (s, W, 130, 59), (s, S)], data)
    assert digests(got) == [hashlib.sha256(data[:130]).digest(), hashlib.sha256(data[:189]).digest()]
    hs.close()


def test_sum_reset_and_reset_restart_from_the_empty_hash(engine):
    data = np.random.default_rng(24).bytes(200)
    hs = HashStreams(engine, 3)
    got = hs.run([(0, W, 0, 100), (0, SR), (0, S), (0, W, 100, 57), (0, S),
                  (1, W, 0, 63), (1, R), (1, S), (1, W, 3, 64), (1, SR), (1, SR),
                  (2, W, 0, 200)], data)
    assert digests(got) == [hashlib.sha256(data[:100]).digest(), EMPTY, hashlib.sha256(data[100:157]).digest(),
                            EMPTY, hashlib.sha256(data[3:67]).digest(), EMPTY]
    # across calls: a Reset alone, then a Sum
    hs.run([(2, R)])
    assert hs.run([(0, R), (0, S), (2, S)])[1].tobytes() == EMPTY
    hs.close()


# ---- state across calls --------------------------------------------------------------------
def test_a_message_cut_into_writes_over_several_calls(engine):
    rng = np.random.default_rng(25)
    msg = rng.bytes(5000)
    cuts = np.sort(rng.integers(0, 5001, 39))
    cuts[5] = cuts[4]
    cuts[20] = cuts[19]  # empty writes
    bounds = [0] + cuts.tolist() + [5000]
    writes = [(bounds[i], bounds[i + 1] - bounds[i]) for i in range(40)]
    assert any(n == 0 for _, n in writes)
    hs = HashStreams(engine, 2)
    for call in np.array_split(np.arange(40), 7):
        hs.run([(1, W, writes[i][0], writes[i][1]) for i in call], msg)
    assert hs.run([(1, S)])[0].tobytes() == hashlib.sha256(msg).digest()
    got = hs.run([(0, W, 100 + i, 1) for i in range(200)] + [(0, S)], msg)
    assert got[0].tobytes() == hashlib.sha256(msg[100:300]).digest()
    hs.close()


# ---- divergent lanes -----------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 64, 65, 257])
def test_one_long_stream_beside_short_ones(engine, n_streams):
    rng = np.random.default_rng(26 + n_streams)
    arena = rng.bytes(300 * 64 + 3 + 200)
    hs = HashStreams(engine, n_streams)
    long_one = min(17, n_streams - 1)
    idle = [s for s in range(n_streams) if s % 5 == 4 and s != long_one]  # no op names them below
    before = {s: rng.bytes(int(rng.integers(1, 100))) for s in idle}
    if idle:
        hs.run([(s, W, sum(len(before[t]) for t in idle[:k]), len(before[s])) for k, s in enumerate(idle)],
               b"".join(before[s] for s in idle))
    ops, want = [], []
    for s in range(n_streams):
        if s in before:
            continue
        if s == long_one:
            off, n = 1, 300 * 64 + 3
        else:
            n = int(rng.integers(0, 131))  # 0-2 blocks; 0: a stream named by a zero-length write and a Sum
            off = int(rng.integers(0, len(arena) - n))
        ops += [(s, W, off, n), (s, S)]
        want.append(hashlib.sha256(arena[off:off + n]).digest())
    assert digests(hs.run(ops, arena)) == want
    # streams that no op named sum to their earlier value
    assert digests(hs.run([(s, S) for s in idle])) == [hashlib.sha256(before[s]).digest() for s in idle]
    hs.close()


# ---- 64-bit length, export / import ------------------------------------------------------------
K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
     0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
     0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
     0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
     0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
     0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
     0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
     0xc67178f2]
H0 = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
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


def continued(h, buffered, length, more):
    """Sum of a state (h, buffered bytes, total length) after Write(more)."""
    total = length + len(more)
    tail = buffered + more + b"\x80"
    tail += bytes(-(len(tail) + 8) % 64) + struct.pack(">Q", 8 * total)
    for i in range(0, len(tail), 64):
        h = compress(h, tail[i:i + 64])
    return struct.pack(">8I", *h)


def marshal(h, buffered, length):
    return b"sha\x03" + struct.pack(">8I", *h) + buffered.ljust(64, b"\0") + struct.pack(">Q", length)


def test_plain_python_compression_is_sha256():
    assert continued(H0, b"", 0, b"abc") == hashlib.sha256(b"abc").digest()
    assert continued(H0, b"", 0, bytes(200)) == hashlib.sha256(bytes(200)).digest()


def test_bit_length_is_64_bit(engine):
    rng = np.random.default_rng(27)
    more = rng.bytes(100)
    cases = [([int(x) for x in rng.integers(0, 1 << 32, 8)], b"", (1 << 32) - 64),
             ([int(x) for x in rng.integers(0, 1 << 32, 8)], rng.bytes(5), (1 << 35) + 5)]
    hs = HashStreams(engine, 2)
    hs.import_state([0, 1], b"".join(marshal(*c) for c in cases))
    got = hs.run([(0, W, 0, 100), (0, S), (1, W, 0, 100), (1, S)], more)
    assert digests(got) == [continued(h, buf, n, more) for h, buf, n in cases]
    hs.close()


def test_export_is_the_hand_built_state_and_import_is_its_inverse(engine):
    data = np.random.default_rng(28).bytes(400)
    hs = HashStreams(engine, 3)
    assert hs.export_state([2])[0].tobytes() == marshal(H0, b"", 0)
    hs.run([(0, W, 0, 30), (0, W, 30, 37), (0, S)], data)  # 67 bytes: one block, 3 buffered
    state = hs.export_state([0, 2])
    assert state[0].tobytes() == marshal(compress(H0, data[:64]), data[64:67], 67)
    assert state[1].tobytes() == marshal(H0, b"", 0)
    hs.import_state([1], state[:1])
    got = hs.run([(0, W, 67, 200), (1, W, 67, 200), (0, S), (1, S), (1, W, 267, 133), (1, S)], data)
    assert digests(got) == [hashlib.sha256(data[:267]).digest()] * 2 + [hashlib.sha256(data).digest()]
    # a wrong magic is refused and changes nothing
    bad = bytearray(state[:1].tobytes())
    bad[3] = 2
    with pytest.raises(MirshaError) as e:
        hs.import_state([2, 0], marshal(H0, b"", 0) + bytes(bad))
    assert e.value.code == _lib.MIRSHA_EINVAL
    assert hs.run([(0, S)])[0].tobytes() == hashlib.sha256(data[:267]).digest()
    hs.close()


# ---- cross-checks --------------------------------------------------------------------------
def test_digest_programmes_give_the_checkpoint_chains_values(engine):
    rng = np.random.default_rng(29)
    n, m = 5, 40
    table = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    chains, hs = CheckpointChains(engine, n), HashStreams(engine, n)
    for _ in range(3):  # state carries over the calls on both
        op_chain = rng.integers(0, n, 120).astype(np.uint32)
        op_digest = rng.integers(0, m, 120).astype(np.uint32)
        op_digest[rng.random(120) < 0.1] = _lib.MIRSHA_NULL_INDEX
        op_digest[rng.random(120) < 0.15] = _lib.MIRSHA_COMMIT_CHECKPOINT
        ops = []
        for c, d in zip(op_chain.tolist(), op_digest.tolist()):
            if d == _lib.MIRSHA_COMMIT_CHECKPOINT:
                ops.append((c, SR))
            else:  # a null request's Write changes nothing: a zero-length write
                ops.append((c, W, 0, 0) if d == _lib.MIRSHA_NULL_INDEX else (c, W, 32 * d, 32))
        assert np.array_equal(hs.run(ops, table), chains.commit(table, op_chain, op_digest))
    chains.close()
    hs.close()


def commit_cycle(rng):
    commits = []
    for seq in range(1, 9):
        ds = [rng.bytes(32) for _ in range(int(rng.integers(1, 6)))]
        ds[int(rng.integers(0, len(ds)))] = None if seq % 2 else b""  # null requests
        commits.append(Commit(batch=CommitBatch(digests=ds, seq_no=seq)))
        if seq in (3, 8):
            commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
    return commits


def test_stream_log_in_a_processor_equals_device_log(engine):
    commits = commit_cycle(np.random.default_rng(30))
    a, b = StreamLog(engine, 4, node=2), DeviceLog(engine, 4, node=2)
    ra = Processor(engine, log=a).process(Actions(commits=commits))
    rb = Processor(engine, log=b).process(Actions(commits=commits))
    assert len(ra.checkpoints) == 2
    assert [c.value for c in ra.checkpoints] == [c.value for c in rb.checkpoints]
    assert [c.checkpoint for c in ra.checkpoints] == [c.checkpoint for c in rb.checkpoints]
    assert np.array_equal(a.values, b.values) and a.values.shape == (2, 4, 32)
    # the four nodes' writes name the same ranges: the cycle's bytes are sent once
    assert a.streams.bytes_sent == sum(len(d) for c in commits if c.batch for d in c.batch.digests if d)
    # a second cycle continues both logs (the cycle ends behind a checkpoint: from the empty hash)
    more = commits[:3]
    assert a.commit_cycle(more) == b.commit_cycle(more) == []
    tail = [Commit(checkpoint=Checkpoint(seq_no=9))]
    assert a.commit_cycle(tail) == b.commit_cycle(tail)
    a.close()
    b.close()


def test_stream_log_with_application_defined_entry_data(engine):
    commits = commit_cycle(np.random.default_rng(31))

    def entry_data(batch):
        return [uint64_to_bytes(batch.seq_no)] + [d for d in batch.digests if d]

    log = StreamLog(engine, 3, node=1, entry_data=entry_data)
    got = Processor(engine, log=log).process(Actions(commits=commits)).checkpoints
    want, ref = [], hashlib.sha256()
    for c in commits:
        if c.checkpoint is not None:
            want.append(ref.digest())
            ref = hashlib.sha256()
        else:
            ref.update(b"".join(entry_data(c.batch)))
    assert [c.value for c in got] == want and len(want) == 2
    assert all(np.array_equal(log.values[:, k], log.values[:, 0]) for k in range(3))
    log.close()


# ---- hashers -------------------------------------------------------------------------------
def test_a_hundred_hashers_flush_in_one_launch(engine):
    rng = np.random.default_rng(32)
    hs = HashStreams(engine, 100)
    hashers = [hs.hasher() for _ in range(100)]
    want = []
    for h in hashers:
        chunks = [rng.bytes(int(rng.integers(0, 150))) for _ in range(3)]
        assert [h.write(c) for c in chunks] == [len(c) for c in chunks]
        want.append(hashlib.sha256(b"".join(chunks)).digest())
    engine.set_timing_mask([KERNEL_STREAMS])
    engine.set_timing(True)
    engine.reset_timing()
    try:
        got = hs.flush(hashers)
        launches, _ = engine.kernel_time(KERNEL_STREAMS)
    finally:
        engine.set_timing(False)
        engine.set_timing_mask(range(32))
    assert got == want and launches == 1 and hs.runs == 1
    with pytest.raises(MirshaError):
        hs.hasher()  # all in use
    freed = hashers[7].stream
    hashers[7].close()
    h = hs.hasher()  # a released stream comes back as Hasher()
    assert h.stream == freed and h.sum() == EMPTY and h.size == 32 and h.block_size == 64
    hs.close()


def test_a_hasher_summed_after_every_write_sends_each_byte_once(engine):
    rng = np.random.default_rng(33)
    hs = HashStreams(engine, 2)
    h, old = hs.hasher(), GpuHash(engine)
    ref, total = hashlib.sha256(), 0
    for k in range(10):
        chunk = rng.bytes(int(rng.integers(1, 300)))
        h.write(chunk)
        old.write(chunk)
        ref.update(chunk)
        total += len(chunk)
        assert h.sum() == ref.digest() == old.sum()
        assert h.sum(b"pre") == b"pre" + ref.digest()  # Sum appends; nothing new is sent
        assert hs.bytes_sent == total, k
    h.reset()
    assert h.sum() == EMPTY
    h.write(b"abc")
    assert h.sum() == hashlib.sha256(b"abc").digest() and hs.bytes_sent == total + 3
    hs.close()


# ---- refused calls -------------------------------------------------------------------------
def test_refused_calls_leave_every_state_untouched(engine):
    data = np.random.default_rng(34).bytes(128)
    hs = HashStreams(engine, 4)
    hs.run([(s, W, s, 40 + s) for s in range(4)], data)
    want = [hashlib.sha256(data[s:s + 40 + s]).digest() for s in range(4)]
    good = [(0, W, 0, 64), (1, SR), (2, R)]
    for bad, word in (((4, W, 0, 1), "op_stream[3]"), ((0, 4, 0, 0), "op_kind[3]"), ((3, W, 100, 29), "op 3"),
                      ((3, W, 129, 0), "op 3")):
        with pytest.raises(MirshaError) as e:
            hs.run(good + [bad] + good, data)
        assert e.value.code == _lib.MIRSHA_EINVAL and word in str(e.value), str(e.value)
    other = HashStreams(engine, 1)
    with pytest.raises(MirshaError):
        other.run([(1, S)])
    other.close()
    with pytest.raises(MirshaError):
        hs.export_state([4])
    assert hs.run([]).shape == (0, 32)  # n_ops == 0 is valid
    assert digests(hs.run([(s, S) for s in range(4)])) == want
    hs.close()
