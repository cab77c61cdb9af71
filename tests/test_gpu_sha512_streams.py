"""Streaming hash states under SHA-512/256 (mirsha_streams_create_hasher and the
kernels of mirsha_sha512_streams.hip; HashStreams(hasher=...), its hash.Hash
form and StreamLog): Write / Sum / Reset over any bytes when the node's Hasher
is sha512.New512_256, bit-exact against hashlib; states against the
plain-Python compression of tests/stream512ref.py.  Never against the code
under test.  Every case is one or a few launches over a few KB: the shapes are
every fill of the 128-byte block against the lengths around its edges, every
arena alignment, wave edges."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, Actions, Checkpoint, Commit,
                        CommitBatch, DeviceLog, Engine, HashStreams, MirshaError, Processor, StreamLog, _lib)
from mirbft_amd.engine import KERNEL_STREAMS
from mirbft_amd.hashdata import uint64_to_bytes

import stream512ref as ref

pytestmark = pytest.mark.gpu

NAME = "sha512_256"
EMPTY = bytes.fromhex("c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a")
W, S, SR, R = STREAM_WRITE, STREAM_SUM, STREAM_SUM_RESET, STREAM_RESET


def H(b) -> bytes:
    return hashlib.new(NAME, bytes(b)).digest()


@pytest.fixture(scope="module")
def own(engine):
    """An engine of this module's own (after the session's, so torch's runtime
    came up first): a failing test cannot leave the shared one on SHA-512/256."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def eng(own):
    own.set_hasher(NAME)
    yield own
    own.set_hasher("sha256")


def digests(rows):
    return [r.tobytes() for r in rows]


def cuda_bytes(data, lead=0):
    """`data` in device memory `lead` bytes into an allocation: (tensor, address)."""
    import torch

    t = torch.frombuffer(bytearray(bytes(lead) + bytes(data)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead


# ---- fill x length: one stream per (b, L), Write(b bytes), Write(L bytes), Sum ----------
GRID = [(b, L) for b in range(128)
        for L in sorted({n for n in (0, 1, 127 - b, 128 - b, 129 - b, 128, 129, 255, 256, 257) if n >= 0})]
POOL = np.random.default_rng(0x512).integers(0, 256, len(GRID) + 600, dtype=np.uint8).tobytes()


def fl_parts(s):
    """Stream s = GRID[s]: its two writes' bytes (content differs per stream)."""
    b, L = GRID[s]
    return POOL[s:s + b], POOL[s + 177:s + 177 + L]


_fl_want = []


def fl_want():
    """The hashlib digests of the fill x length streams: computed once, shared."""
    if not _fl_want:
        _fl_want.append([H(b"".join(fl_parts(s))) for s in range(len(GRID))])
    return _fl_want[0]


def fl_programme(align=None):
    """(ops, arena): with `align` the L-byte range of every stream starts at an
    arena offset = align (mod 16), else the ranges lie back to back."""
    n = len(GRID)
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


def test_fill_times_length_in_one_run(eng):
    assert len(GRID) > 1000
    hs = HashStreams(eng, len(GRID))
    assert hs.hasher == NAME
    ops, arena = fl_programme()
    assert digests(hs.run(ops, arena)) == fl_want()
    hs.close()


@pytest.mark.parametrize("align", range(16))
def test_fill_times_length_at_every_arena_alignment(eng, align):
    """The device form reads the arena where it lies, so the L-byte range really
    sits at that alignment (the host form packs the written bytes)."""
    hs = HashStreams(eng, len(GRID))
    ops, arena = fl_programme(align)
    assert all(int(o) % 16 == align for o in ops[2][1::3])
    t, at = cuda_bytes(arena)
    assert digests(hs.run_device(ops, at, len(arena))) == fl_want()
    hs.close()


def test_fill_times_length_from_a_tensor_at_an_odd_address(eng):
    ops, arena = fl_programme()
    for lead in (0, 1, 3):
        hs = HashStreams(eng, len(GRID))
        t, at = cuda_bytes(arena, lead)
        assert at % 4 == lead
        assert digests(hs.run_device(ops, at, len(arena))) == fl_want(), lead
        hs.close()


# ---- arena edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_form", [False, True])
def test_write_range_at_arena_offset_0_arriving_at_a_fill(eng, device_form):
    """The stream-aligned window of such a write begins before the arena."""
    rng = np.random.default_rng(121)
    fills, lens = (1, 3, 17, 64, 126, 127), (1, 2, 61, 128, 200)
    hs = HashStreams(eng, len(fills) * len(lens))
    heads = {f: rng.bytes(f) for f in fills}
    hs.run([(k * len(lens) + j, W, sum(fills[:k]), f) for k, f in enumerate(fills) for j in range(len(lens))],
           b"".join(heads[f] for f in fills))
    for j, L in enumerate(lens):  # one run per length: every fill's stream takes the arena's first L bytes
        body = rng.bytes(L)
        ops = [op for k in range(len(fills)) for op in ((k * len(lens) + j, W, 0, L), (k * len(lens) + j, S))]
        if device_form:
            t, at = cuda_bytes(body, j % 4)
            got = hs.run_device(ops, at, L)
        else:
            got = hs.run(ops, body)
        assert digests(got) == [H(heads[f] + body) for f in fills], L
    hs.close()


@pytest.mark.parametrize("device_form", [False, True])
def test_write_ranges_ending_at_the_arenas_last_byte(eng, device_form):
    rng = np.random.default_rng(122)
    A = 331  # not a multiple of 4
    arena = rng.bytes(A)
    lens = list(range(1, 140)) + [255, 256, 257, 331]
    hs = HashStreams(eng, len(lens) + 1)
    ops = [(len(lens), W, 0, 1)]  # the host form's packed bytes are no multiple of 4 either
    for s, L in enumerate(lens):
        ops += [(s, W, A - L, L), (s, S)]
    if device_form:
        t, at = cuda_bytes(arena, 1)
        got = hs.run_device(ops, at, A)
    else:
        got = hs.run(ops, arena)
    assert digests(got) == [H(arena[A - L:]) for L in lens]
    hs.close()


# ---- padding edges -------------------------------------------------------------------------
def test_padding_edges_and_sum_leaves_the_state(eng):
    rng = np.random.default_rng(123)
    totals = (0, 1, 111, 112, 113, 127, 128, 239, 240, 256)
    data = rng.bytes(600)
    hs = HashStreams(eng, len(totals) + 1)
    ops = []
    for s, n in enumerate(totals):
        ops += [(s, W, 7, n), (s, S), (s, S)]
    assert digests(hs.run(ops, data)) == [H(data[7:7 + n]) for n in totals for _ in range(2)]
    # the states are as they were: written on in another call and summed again
    ops = []
    for s, n in enumerate(totals):
        ops += [(s, S), (s, W, 7 + n, 150), (s, S)]
    assert digests(hs.run(ops, data)) == [H(data[7:7 + n + k]) for n in totals for k in (0, 150)]
    s = len(totals)
    got = hs.run([(s, W, 0, 120), (s, S), (s, W, 120, 70), (s, S), (s, S)], data)
    assert digests(got) == [H(data[:120])] + [H(data[:190])] * 2
    hs.close()


def test_sum_reset_and_reset_restart_from_the_empty_hash(eng):
    data = np.random.default_rng(124).bytes(400)
    hs = HashStreams(eng, 3)
    got = hs.run([(0, W, 0, 200), (0, SR), (0, S), (0, W, 200, 115), (0, S),
                  (1, W, 0, 127), (1, R), (1, S), (1, W, 3, 128), (1, SR), (1, SR),
                  (2, W, 0, 400)], data)
    assert digests(got) == [H(data[:200]), EMPTY, H(data[200:315]), EMPTY, H(data[3:131]), EMPTY]
    hs.run([(2, R)])  # across calls: a Reset alone, then a Sum
    assert hs.run([(0, R), (0, S), (2, S)])[1].tobytes() == EMPTY
    hs.close()


# ---- state across calls --------------------------------------------------------------------
def test_a_message_cut_into_writes_over_several_calls(eng):
    rng = np.random.default_rng(125)
    msg = rng.bytes(5000)
    cuts = np.sort(rng.integers(0, 5001, 39))
    cuts[5] = cuts[4]
    cuts[20] = cuts[19]  # empty writes
    bounds = [0] + cuts.tolist() + [5000]
    writes = [(bounds[i], bounds[i + 1] - bounds[i]) for i in range(40)]
    assert any(n == 0 for _, n in writes)
    hs = HashStreams(eng, 2)
    for call in np.array_split(np.arange(40), 7):
        hs.run([(1, W, writes[i][0], writes[i][1]) for i in call], msg)
    assert hs.run([(1, S)])[0].tobytes() == H(msg)
    got = hs.run([(0, W, 100 + i, 1) for i in range(300)] + [(0, S)], msg)
    assert got[0].tobytes() == H(msg[100:400])
    hs.close()


# ---- divergent lanes -----------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 64, 65, 257])
def test_one_long_stream_beside_short_ones(eng, n_streams):
    rng = np.random.default_rng(126 + n_streams)
    arena = rng.bytes(300 * 128 + 3 + 300)
    hs = HashStreams(eng, n_streams)
    long_one = min(17, n_streams - 1)
    idle = [s for s in range(n_streams) if s % 5 == 4 and s != long_one]  # no op names them below
    before = {s: rng.bytes(int(rng.integers(1, 200))) for s in idle}
    if idle:
        hs.run([(s, W, sum(len(before[t]) for t in idle[:k]), len(before[s])) for k, s in enumerate(idle)],
               b"".join(before[s] for s in idle))
    ops, want = [], []
    for s in range(n_streams):
        if s in before:
            continue
        if s == long_one:
            off, n = 1, 300 * 128 + 3
        else:
            n = int(rng.integers(0, 260))  # 0-2 blocks; 0: a stream named by a zero-length write and a Sum
            off = int(rng.integers(0, len(arena) - n))
        ops += [(s, W, off, n), (s, S)]
        want.append(H(arena[off:off + n]))
    assert digests(hs.run(ops, arena)) == want
    assert digests(hs.run([(s, S) for s in idle])) == [H(before[s]) for s in idle]
    hs.close()


# ---- the length, export / import -----------------------------------------------------------
def test_bit_length_beyond_32_bits(eng):
    """Hand-built states whose lengths are 2^32 + 100 and 2^40 + 111: the padded
    bit length has to carry beyond 32 and beyond 40 bits."""
    rng = np.random.default_rng(127)
    more = rng.bytes(150)
    cases = [([int(x) for x in rng.integers(0, 1 << 63, 8)], rng.bytes(100), (1 << 32) + 100),
             ([int(x) for x in rng.integers(0, 1 << 63, 8)], rng.bytes(111), (1 << 40) + 111)]
    assert all(len(buf) == n % 128 for _, buf, n in cases)
    hs = HashStreams(eng, 2)
    hs.import_state([0, 1], b"".join(ref.marshal(*c) for c in cases))
    got = hs.run([(0, S), (0, W, 0, 150), (0, S), (1, W, 0, 150), (1, S)], more)
    want = [ref.continue_from(*cases[0], b""), ref.continue_from(*cases[0], more), ref.continue_from(*cases[1], more)]
    assert digests(got) == want
    hs.close()


def test_export_is_the_hand_built_state_and_import_is_its_inverse(eng):
    data = np.random.default_rng(128).bytes(700)
    hs = HashStreams(eng, 3)
    assert hs.state_bytes == 204
    assert hs.export_state([2])[0].tobytes() == ref.marshal(ref.H0, b"", 0)
    hs.run([(0, W, 0, 30), (0, W, 30, 101), (0, S)], data)  # 131 bytes: one block, 3 buffered
    state = hs.export_state([0, 2])
    assert state.shape == (2, 204)
    assert state[0].tobytes() == ref.marshal(ref.compress(list(ref.H0), data[:128]), data[128:131], 131)
    assert state[0].tobytes() == ref.marshal_of(data[:131])
    assert state[1].tobytes() == ref.marshal(ref.H0, b"", 0)
    hs.import_state([1], state[:1])
    got = hs.run([(0, W, 131, 300), (1, W, 131, 300), (0, S), (1, S), (1, W, 431, 269), (1, S)], data)
    assert digests(got) == [H(data[:431])] * 2 + [H(data)]
    # a wrong magic is refused and changes nothing: a SHA-256 state's magic among them
    for magic in (b"sha\x03", b"sha\x07"):
        bad = magic + state[0].tobytes()[4:]
        with pytest.raises(MirshaError) as e:
            hs.import_state([2, 0], ref.marshal(ref.H0, b"x", 1) + bad)
        assert e.value.code == _lib.MIRSHA_EINVAL
    assert digests(hs.run([(0, S), (2, S)])) == [H(data[:431]), EMPTY]
    hs.close()


def test_sha256_streams_refuse_a_sha512_state(eng):
    eng.set_hasher("sha256")
    hs = HashStreams(eng, 1)
    assert hs.hasher == "sha256" and hs.state_bytes == 108
    hs.run([(0, W, 0, 3)], b"abc")
    with pytest.raises(MirshaError) as e:
        hs.import_state([0], b"sha\x06" + bytes(104))
    assert e.value.code == _lib.MIRSHA_EINVAL
    assert hs.run([(0, S)])[0].tobytes() == hashlib.sha256(b"abc").digest()
    hs.close()


# ---- refusals ------------------------------------------------------------------------------
def _calls(hs, data):
    return (lambda: hs.run([(0, W, 0, 3), (0, S)], data), lambda: hs.submit([(0, W, 0, 3), (0, S)], data),
            lambda: hs.export_state([0]), lambda: hs.import_state([0], bytes(hs.state_bytes)))


@pytest.mark.parametrize("streams_hasher", ["sha512_256", "sha256"])
def test_streams_under_the_other_hasher_are_refused_and_untouched(own, streams_hasher):
    other = "sha256" if streams_hasher == NAME else NAME
    new = hashlib.sha256 if streams_hasher == "sha256" else (lambda b=b"": hashlib.new(NAME, b))
    data = np.random.default_rng(129).bytes(300)
    try:
        own.set_hasher(streams_hasher)
        hs = HashStreams(own, 2)
        assert hs.hasher == streams_hasher
        hs.run([(0, W, 0, 200), (1, W, 5, 77)], data)
        before = hs.export_state([0, 1])
        t = own.submit_slices([[b"ring"]])  # a ticket in flight: the ring is left as it is
        own.set_hasher(other)
        for refused in _calls(hs, data):
            with pytest.raises(MirshaError) as ei:
                refused()
            msg = str(ei.value)
            assert ei.value.code == _lib.MIRSHA_EINVAL and "sha512_256" in msg and "sha256" in msg, msg
            assert "mirsha_streams_" in msg, msg
        t2 = own.submit_slices([[b"ring2"]])
        assert t2.value == t.value + 1  # the refused submissions took no ticket
        own.wait(t2)
        own.set_hasher(streams_hasher)  # the same object is served once the context is set back
        assert np.array_equal(hs.export_state([0, 1]), before)
        assert digests(hs.run([(0, S), (1, S)])) == [new(data[:200]).digest(), new(data[5:82]).digest()]
        hs.close()
    finally:
        own.set_hasher("sha256")


def test_unknown_hasher_is_refused_and_both_kinds_coexist(own):
    import ctypes

    out = ctypes.c_void_p()
    rc = own._lib.mirsha_streams_create_hasher(own.ctx, 1, 7, ctypes.byref(out))
    assert rc == _lib.MIRSHA_EINVAL and not out.value
    with pytest.raises(ValueError):
        HashStreams(own, 1, hasher="sha1")
    a, b = HashStreams(own, 2, hasher="sha256"), HashStreams(own, 2, hasher=NAME)
    assert (a.hasher, b.hasher) == ("sha256", NAME)
    assert own._lib.mirsha_streams_hasher(a.handle) == _lib.MIRSHA_HASHER_SHA256
    assert own._lib.mirsha_streams_hasher(b.handle) == _lib.MIRSHA_HASHER_SHA512_256
    data = bytes(range(200))
    ops = [(1, W, 0, 130), (1, S), (0, W, 3, 70), (0, S)]
    try:
        for _ in range(2):  # alternately, each with its own state
            own.set_hasher("sha256")
            ga = digests(a.run(ops, data))
            own.set_hasher(NAME)
            gb = digests(b.run(ops, data))
        assert ga == [hashlib.sha256(data[:130] * 2).digest(), hashlib.sha256(data[3:73] * 2).digest()]
        assert gb == [H(data[:130] * 2), H(data[3:73] * 2)]
    finally:
        own.set_hasher("sha256")
        a.close()
        b.close()


# ---- the log and the hashers ---------------------------------------------------------------
def commit_cycle(rng):
    commits = []
    for seq in range(1, 9):
        ds = [rng.bytes(32) for _ in range(int(rng.integers(1, 6)))]
        ds[int(rng.integers(0, len(ds)))] = None if seq % 2 else b""  # null requests
        commits.append(Commit(batch=CommitBatch(digests=ds, seq_no=seq)))
        if seq in (3, 8):
            commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
    return commits


def hashlib_checkpoints(commits, entry_data):
    want, h = [], hashlib.new(NAME)
    for c in commits:
        if c.checkpoint is not None:
            want.append(h.digest())
            h = hashlib.new(NAME)
        else:
            h.update(b"".join(entry_data(c.batch)))
    return want


@pytest.mark.parametrize("async_commits", [False, True])
def test_stream_log_under_a_sha512_processor_equals_device_log_and_hashlib(own, async_commits):
    commits = commit_cycle(np.random.default_rng(130))
    try:
        pa = Processor(own, hasher=NAME, async_commits=async_commits)
        pa.log = a = StreamLog(own, 4, node=2)  # made after the Processor set the hasher
        pb = Processor(own, log=DeviceLog(own, 4, node=2, hasher=NAME), async_commits=async_commits)
        assert a.streams.hasher == NAME
        run = (lambda p, a: p.submit(a).wait()) if async_commits else (lambda p, a: p.process(a))
        ra, rb = run(pa, Actions(commits=commits)), run(pb, Actions(commits=commits))
        want = hashlib_checkpoints(commits, lambda batch: [d for d in batch.digests if d])
        assert [c.value for c in ra.checkpoints] == [c.value for c in rb.checkpoints] == want and len(want) == 2
        assert np.array_equal(a.values, pb.log.values) and a.values.shape == (2, 4, 32)
        a.close()
        pb.log.close()
        # a log whose streams hash with another function than the engine raises at the first commit
        stale = StreamLog(own, 1, hasher="sha256")
        with pytest.raises(MirshaError) as e:
            stale.commit_cycle(commits)
        assert e.value.code == _lib.MIRSHA_EINVAL
        stale.close()
    finally:
        own.set_hasher("sha256")


def test_processor_log_argument_and_application_defined_entry_data(eng):
    commits = commit_cycle(np.random.default_rng(131))

    def entry_data(batch):  # 8 + 32 k bytes: never a multiple of 32
        return [uint64_to_bytes(batch.seq_no)] + [d for d in batch.digests if d]

    for async_commits in (False, True):
        log = StreamLog(eng, 3, node=1, entry_data=entry_data)
        p = Processor(eng, log=log, async_commits=async_commits)
        got = (p.submit(Actions(commits=commits)).wait() if async_commits else p.process(Actions(commits=commits))).checkpoints
        assert [c.value for c in got] == hashlib_checkpoints(commits, entry_data) and len(got) == 2
        assert all(np.array_equal(log.values[:, k], log.values[:, 0]) for k in range(3))
        log.close()


def test_a_hundred_hashers_flush_in_one_launch(eng):
    rng = np.random.default_rng(132)
    hs = HashStreams(eng, 100)
    hashers = [hs.hasher() for _ in range(100)]
    want = []
    for h in hashers:
        chunks = [rng.bytes(int(rng.integers(0, 300))) for _ in range(3)]
        assert [h.write(c) for c in chunks] == [len(c) for c in chunks]
        want.append(H(b"".join(chunks)))
    eng.set_timing_mask([KERNEL_STREAMS])
    eng.set_timing(True)
    eng.reset_timing()
    try:
        got = hs.flush(hashers)
        launches, _ = eng.kernel_time(KERNEL_STREAMS)
    finally:
        eng.set_timing(False)
        eng.set_timing_mask(range(32))
    assert got == want and launches == 1 and hs.runs == 1
    freed = hashers[7].stream
    hashers[7].close()
    h = hs.hasher()  # a released stream comes back as Hasher()
    assert h.stream == freed and h.sum() == EMPTY and (h.size, h.block_size) == (32, 128)
    h.write(b"abc")
    assert h.sum(b"pre") == b"pre" + H(b"abc")
    hs.close()
