"""Engine: one gfx950 device context behind the C-ABI (include/mirsha.h).

Host-memory entry points take numpy arrays / bytes and return numpy digests
``(n, 32) uint8`` in ORIGIN order.  Device-pointer entry points take raw device
addresses (ints, e.g. ``torch.Tensor.data_ptr()``) and are asynchronous on the
engine's stream.  Every call runs the HIP kernels; there is no CPU path here.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import MIRSHA_COMMIT_CHECKPOINT, MIRSHA_NULL_INDEX, MirshaError, check

KERNEL_MSGS = 0
KERNEL_LISTS = 1
KERNEL_GEN = 2
KERNEL_CHAIN = 3
KERNEL_FUSED = 4
KERNEL_OVERLAP = 5
KERNEL_VERIFY = 6
KERNEL_EXPECT = 7
KERNEL_ORDER = 8
KERNEL_STREAMS = 9
# op kinds of a stream programme (mirsha_streams_run)
STREAM_WRITE = _lib.MIRSHA_STREAM_WRITE
STREAM_SUM = _lib.MIRSHA_STREAM_SUM
STREAM_SUM_RESET = _lib.MIRSHA_STREAM_SUM_RESET
STREAM_RESET = _lib.MIRSHA_STREAM_RESET
ORDER_MODES = {"host": _lib.MIRSHA_ORDER_HOST, "device": _lib.MIRSHA_ORDER_DEVICE}
# The Processor's `Hasher` (processor.go:21,58): sha256.New or sha512.New512_256.
HASHERS = {"sha256": _lib.MIRSHA_HASHER_SHA256, "sha512_256": _lib.MIRSHA_HASHER_SHA512_256}
ASYNC_SLOTS = 4  # submissions in flight per context (mirsha_submit_slices)

# mirsha_pipeline modes (include/mirsha.h)
PIPELINE_SEQUENTIAL = 0
PIPELINE_FUSED = 1
PIPELINE_AUTO = 3
PIPELINE_MODES = {"sequential": PIPELINE_SEQUENTIAL, "fused": PIPELINE_FUSED, "auto": PIPELINE_AUTO}
VARIANT_LDS = 0
VARIANT_DIRECT = 1
VARIANT_LOWOCC = 4
VARIANT_LDS_ONLY = 5
VARIANT_PAIR = 6
VARIANT_CU = 10
VARIANTS = (VARIANT_LDS, VARIANT_DIRECT, VARIANT_LOWOCC, VARIANT_LDS_ONLY, VARIANT_PAIR, VARIANT_CU)


def _ptr(a: np.ndarray | None) -> int | None:
    if a is None:
        return None
    return a.ctypes.data if a.size else None


def _hasher_id(hasher: str | int) -> int:
    """A hasher's id from its name or id; ValueError for an unknown one (no
    library call)."""
    if isinstance(hasher, str):
        if hasher not in HASHERS:
            raise ValueError(f"hasher {hasher!r}: one of {sorted(HASHERS)}")
        return HASHERS[hasher]
    if int(hasher) not in HASHERS.values():
        raise ValueError(f"hasher {hasher!r}: one of {sorted(HASHERS.values())}")
    return int(hasher)


def hasher_info(hasher: str | int) -> tuple[int, int]:
    """(digest bytes, block bytes) of a hasher, Go's Size() and BlockSize():
    (32, 64) for "sha256", (32, 128) for "sha512_256" (mirsha_hasher_info; host
    only, no device needed)."""
    size, block = ctypes.c_uint32(0), ctypes.c_uint32(0)
    check(_lib.load().mirsha_hasher_info(_hasher_id(hasher), ctypes.byref(size), ctypes.byref(block)))
    return size.value, block.value


def sha512_pair_max_groups() -> int:
    """The largest launch, in 64-lane groups, that takes the producer/consumer
    pair kernels under "sha512_256" (mirsha_sha512_pair_max_groups; host only,
    no device needed).  0: the automatic route is off."""
    return int(_lib.load().mirsha_sha512_pair_max_groups())


def _as_u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf.reshape(-1).view(np.uint8))
    return np.frombuffer(memoryview(buf), dtype=np.uint8)


class SliceArrays:
    """HashRequest.Data of n requests as the C-ABI's slice arrays: slice s is
    ``len[s]`` bytes at address ``ptr[s]``; request i = slices [first[i], first[i+1]).
    Holds references to the Python buffers the pointers come from."""

    def __init__(self, ptr: np.ndarray, length: np.ndarray, first: np.ndarray, keep=()):
        self.ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        self.len = np.ascontiguousarray(length, dtype=np.uint64)
        self.first = np.ascontiguousarray(first, dtype=np.uint32)
        if self.ptr.shape != self.len.shape or self.first.size < 1 or int(self.first[-1]) != self.ptr.size:
            raise ValueError("inconsistent slice arrays")
        self.keep = keep
        self.n = int(self.first.size) - 1
        self.ptr_p = _ptr(self.ptr)
        self.len_p = _ptr(self.len)
        self.first_p = _ptr(self.first)

    @classmethod
    def from_requests(cls, requests: Sequence[Sequence[bytes]]) -> "SliceArrays":
        keep, lens, first = [], [], [0]
        for req in requests:
            for s in req:
                b = bytes(s)
                keep.append(b)
                lens.append(len(b))
            first.append(len(keep))
        ptr = np.zeros(len(keep), dtype=np.uint64)
        for i, b in enumerate(keep):
            if len(b):
                ptr[i] = ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value
        return cls(ptr, np.asarray(lens, dtype=np.uint64), np.asarray(first, dtype=np.uint32), keep)

    @classmethod
    def from_buffer(cls, buf: np.ndarray, slice_off: np.ndarray, slice_len: np.ndarray, first: np.ndarray):
        """Slices that are byte ranges of one numpy buffer (vectorised; for large streams)."""
        b = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
        base = b.ctypes.data
        off = np.ascontiguousarray(slice_off, dtype=np.uint64)
        return cls(np.uint64(base) + off, slice_len, first, (b,))


class Ticket:
    """A submission of Engine.submit_slices; ``out`` receives the digests."""

    def __init__(self, value: int, out: np.ndarray):
        self.value = value
        self.out = out


class ExpectTicket(Ticket):
    """A submission of Engine.submit_slices_expect / submit_batch_expect.
    ``has[i]``: request i carried an expectation.  After ``wait`` (or a ``poll``
    that reports done) ``mismatches`` holds the sorted indices whose digest
    differs from their expectation, and ``out[i]`` the digest of every request
    without an expectation and of every mismatch; the row of a matching
    request is NOT written (its digest equals the expectation passed in).
    ``n_unique``: the distinct requests hashed (submit_slices_expect_dedup), else None."""

    def __init__(self, value: int, out: np.ndarray, has: np.ndarray, bits: np.ndarray, count: np.ndarray,
                 short: np.ndarray, n_unique: int | None = None):
        super().__init__(value, out)
        self.has = has
        self.n_unique = n_unique
        self.mismatches: np.ndarray | None = None
        self._bits, self._count, self._short = bits, count, short

    def _resolve(self) -> None:
        if self.mismatches is not None:
            return
        bad = mismatch_indices(self._bits, self.has.size)
        if bad.size != int(self._count[0]):
            raise MirshaError(_lib.MIRSHA_EHIP, f"expect: bitmap has {bad.size} bits set, count is {self._count[0]}")
        self.mismatches = np.union1d(bad, self._short) if self._short.size else bad


class ValuesTicket(Ticket):
    """A segment ticket: a programme over device-resident hash states.
    ``values`` (= ``out``), shape (k, 32): one row per op that yields a value,
    in op order; complete after ``Engine.wait`` (or a ``poll`` that reports
    done)."""

    @property
    def values(self) -> np.ndarray:
        return self.out


class CommitTicket(ValuesTicket):
    """A submission of CheckpointChains.submit_commit / submit_commit_device:
    one row per checkpoint op."""


class StreamTicket(ValuesTicket):
    """A submission of HashStreams.submit / submit_device / submit_flush: one
    row per STREAM_SUM / STREAM_SUM_RESET op.  A ``submit_flush`` ticket's rows
    are in the order of its hashers."""


def _out_rows(out, n: int) -> np.ndarray:
    """A caller-supplied (n, 32) uint8 result array (checked), or a new one."""
    if out is None:
        return np.empty((n, 32), dtype=np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (n, 32) or not out.flags.c_contiguous \
            or not out.flags.writeable:
        raise ValueError(f"out must be a writeable C-contiguous uint8 array of shape ({n}, 32)")
    return out


def mismatch_indices(bits, n: int) -> np.ndarray:
    """Sorted indices of the set bits of a mismatch bitmap (mirsha_verify_*):
    bit ``i & 63`` of word ``i >> 6`` is item ``i``; only the first n bits count."""
    n = int(n)
    words = np.ascontiguousarray(bits, dtype="<u8").reshape(-1)
    if words.size < (n + 63) // 64:
        raise ValueError(f"{words.size} bitmap words for {n} items")
    if n == 0:
        return np.empty(0, dtype=np.int64)
    flags = np.unpackbits(words[:(n + 63) // 64].view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(flags).astype(np.int64)


def _expected_rows(expected, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The expected digests of a verify call as an (n, 32) uint8 array for the
    device, plus the indices that are a mismatch already on the host: a
    sequence entry whose length is not 32 (bytes.Equal of unequal lengths);
    such an entry goes to the device as 32 zero bytes."""
    if isinstance(expected, np.ndarray):
        if expected.dtype != np.uint8 or expected.shape != (n, 32):
            raise ValueError(f"expected must be a uint8 array of shape ({n}, 32)")
        return np.ascontiguousarray(expected), np.empty(0, dtype=np.int64)
    rows = list(expected)
    if len(rows) != n:
        raise ValueError(f"{len(rows)} expected digests for {n} items")
    bad = [i for i, d in enumerate(rows) if len(d) != 32]
    for i in bad:
        rows[i] = bytes(32)
    arr = np.frombuffer(b"".join(bytes(d) for d in rows), dtype=np.uint8).reshape(n, 32)
    return arr, np.asarray(bad, dtype=np.int64)


def expect_plan(expected) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host-only: the expectation arguments of a mixed submission
    (mirsha_submit_*_expect) from one ``Optional[bytes]`` per request.  Returns
    (expect_of, rows, short): the uint32 indices of the requests that carry an
    expectation, their (m, 32) uint8 rows, and the indices whose expectation is
    not 32 bytes long -- a mismatch already on the host (bytes.Equal of unequal
    lengths), sent to the device as 32 zero bytes (the ``_expected_rows`` rule)."""
    expected = list(expected)
    of = [i for i, e in enumerate(expected) if e is not None]
    rows, short = _expected_rows([expected[i] for i in of], len(of))
    return np.asarray(of, dtype=np.uint32), rows, np.asarray([of[int(k)] for k in short], dtype=np.int64)


def expect_bitmap(expect_of, n: int) -> tuple[np.ndarray, np.ndarray]:
    """Host-only mirsha_expect_plan: (has, base) -- the ceil(n/64)-word bitmap of
    the requests listed in ``expect_of`` and the set bits before each word."""
    of = np.ascontiguousarray(expect_of, dtype=np.uint32)
    words = (int(n) + 63) // 64
    has = np.zeros(words, dtype=np.uint64)
    base = np.zeros(words, dtype=np.uint32)
    check(_lib.load().mirsha_expect_plan(_ptr(of), of.size, int(n), _ptr(has), _ptr(base)))
    return has, base


def dedup_plan(requests) -> tuple[np.ndarray, int]:
    """Host-only dedup plan (mirsha_dedup_plan): rep[i] = smallest j <= i with
    identical request bytes; returns (rep, number of distinct requests)."""
    sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
    rep = np.empty(sl.n, dtype=np.uint32)
    u = ctypes.c_uint32(0)
    rc = _lib.load().mirsha_dedup_plan(sl.ptr_p, sl.len_p, sl.first_p, sl.n, _ptr(rep), ctypes.byref(u))
    check(rc)
    return rep, u.value


def dedup_rows(requests) -> tuple[np.ndarray, int]:
    """Host-only (mirsha_dedup_rows): row[i] = where request i's digest lies among
    the distinct requests' digests of a submit_slices_expect_dedup call (equal
    bytes, equal row); returns (row, number of distinct requests)."""
    sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
    row = np.empty(sl.n, dtype=np.uint32)
    u = ctypes.c_uint32(0)
    check(_lib.load().mirsha_dedup_rows(sl.ptr_p, sl.len_p, sl.first_p, sl.n, _ptr(row), ctypes.byref(u)))
    return row, u.value


def _commit_ops(op_chain, op_digest) -> tuple[np.ndarray, np.ndarray]:
    oc = np.ascontiguousarray(op_chain, dtype=np.uint32).reshape(-1)
    od = np.ascontiguousarray(op_digest, dtype=np.uint32).reshape(-1)
    if oc.size != od.size:
        raise ValueError("one chain id and one digest index (or marker) per op")
    return oc, od


def commit_plan(op_chain, op_digest, n_chains: int, n_digests: int):
    """Host-only mirsha_commit_plan: the arrays ``CheckpointChains.commit`` sends
    to the device for a cycle's commit programme.  Returns (act, efirst, ent,
    n_values): the active chains (ascending), their entry ranges
    ``ent[efirst[k]:efirst[k+1]]`` in op order with null writes removed -- a
    digest index, or ``MIRSHA_COMMIT_ENTRY_CHECKPOINT | row`` with the row of
    the values output -- and the number of checkpoint ops."""
    oc, od = _commit_ops(op_chain, op_digest)
    cap = min(oc.size, int(n_chains))
    act = np.zeros(cap, dtype=np.uint32)
    efirst = np.zeros(cap + 1, dtype=np.uint32)
    ent = np.zeros(oc.size, dtype=np.uint32)
    na, ne, nv, bad = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = _lib.load().mirsha_commit_plan(_ptr(oc), _ptr(od), oc.size, int(n_chains), int(n_digests), _ptr(act),
                                        efirst.ctypes.data, _ptr(ent), ctypes.byref(na), ctypes.byref(ne),
                                        ctypes.byref(nv), ctypes.byref(bad))
    if rc != _lib.MIRSHA_OK:
        where = f"op {bad.value}" if bad.value != 0xFFFFFFFF else "arguments"
        raise MirshaError(rc, f"commit plan: {where}")
    return act[:na.value], efirst[:na.value + 1], ent[:ne.value], nv.value


def commit_seg_plan(op_chain, op_digest, n_chains: int, n_digests: int):
    """Host-only mirsha_commit_seg_plan: ``commit_plan``'s per-chain programmes
    cut after every checkpoint entry, one segment per lane of the ring form
    (``CheckpointChains.submit_commit``).  Returns (seg_chain, sfirst,
    seg_flags, ent, n_values): segment s belongs to chain ``seg_chain[s]`` and
    runs ``ent[sfirst[s]:sfirst[s+1]]`` (commit_plan's entries, unchanged);
    ``seg_flags[s]`` has MIRSHA_COMMIT_SEG_FIRST on the chain's first segment
    (it starts from the stored state, every other one from Hasher()) and
    MIRSHA_COMMIT_SEG_LAST on the one holding the chain's final entry."""
    oc, od = _commit_ops(op_chain, op_digest)
    seg_chain = np.zeros(oc.size, dtype=np.uint32)
    sfirst = np.zeros(oc.size + 1, dtype=np.uint32)
    seg_flags = np.zeros(oc.size, dtype=np.uint32)
    ent = np.zeros(oc.size, dtype=np.uint32)
    ns, na, ne, nv, bad = (ctypes.c_uint32(0) for _ in range(5))
    rc = _lib.load().mirsha_commit_seg_plan(_ptr(oc), _ptr(od), oc.size, int(n_chains), int(n_digests),
                                            _ptr(seg_chain), sfirst.ctypes.data, _ptr(seg_flags), _ptr(ent),
                                            ctypes.byref(ns), ctypes.byref(na), ctypes.byref(ne), ctypes.byref(nv),
                                            ctypes.byref(bad))
    if rc != _lib.MIRSHA_OK:
        where = f"op {bad.value}" if bad.value != 0xFFFFFFFF else "arguments"
        raise MirshaError(rc, f"commit segment plan: {where}")
    return seg_chain[:ns.value], sfirst[:ns.value + 1], seg_flags[:ns.value], ent[:ne.value], nv.value


def device_count() -> int:
    n = ctypes.c_int(0)
    check(_lib.load().mirsha_device_count(ctypes.byref(n)))
    return n.value


class Engine:
    """Batched SHA-256 engine on one MI355X.  Replaces `Hasher` (processor.go:21)."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        ctx = ctypes.c_void_p()
        rc = self._lib.mirsha_ctx_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            raise MirshaError(rc, f"cannot create a gfx950 context on device {device}")
        self.ctx = ctx
        self.device = device
        self.last_unique = 0
        # Output arrays of submissions the library has not retired yet: it
        # writes the digests there inside mirsha_wait / mirsha_poll, or when a
        # later submit retires the oldest of its ASYNC_SLOTS ring slots, so
        # they must outlive a dropped Ticket.
        self._outstanding: dict[int, np.ndarray] = {}

    # ------------------------------------------------------------ lifecycle
    def close(self) -> None:
        if getattr(self, "ctx", None):
            self._lib.mirsha_ctx_destroy(self.ctx)  # no digest is written after this
            self.ctx = None
            self._outstanding = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        check(rc, self.ctx)

    # --------------------------------------------------------------- knobs
    def set_stream(self, stream_ptr: int | None) -> None:
        self._check(self._lib.mirsha_ctx_set_stream(self.ctx, stream_ptr))

    @property
    def stream(self) -> int:
        return self._lib.mirsha_ctx_stream(self.ctx) or 0

    def set_variant(self, variant: int) -> None:
        self._check(self._lib.mirsha_ctx_set_variant(self.ctx, int(variant)))

    def set_order_mode(self, mode: str | int) -> None:
        """Where submit_batch / submit_batch_expect build the bucket order of a
        cycle of several block counts: "host" (default) or "device"
        (mirsha_ctx_set_order_mode)."""
        if isinstance(mode, str):
            if mode not in ORDER_MODES:
                raise ValueError(f"order mode {mode!r}: one of {sorted(ORDER_MODES)}")
            mode = ORDER_MODES[mode]
        self._check(self._lib.mirsha_ctx_set_order_mode(self.ctx, int(mode)))

    @property
    def order_mode(self) -> str:
        m = self._lib.mirsha_ctx_order_mode(self.ctx)
        if m < 0:
            self._check(m)
        return {v: k for k, v in ORDER_MODES.items()}[m]

    def set_hasher(self, hasher: str | int) -> None:
        """The hash function of the calls made from now on: "sha256" (default)
        or "sha512_256" (mirsha_ctx_set_hasher; the reference's `Hasher`,
        processor.go:21,58).  The hash, verify and ring calls honour it.
        Checkpoint chains and hash streams carry the hasher they were created
        with (CheckpointChains, DeviceLog; HashStreams, StreamLog) and raise
        MirshaError (MIRSHA_EINVAL) while the engine hashes with another one;
        so do the device plans (``pipeline(..., hasher=...)``; without
        ``hasher`` a plan is SHA-256 and its creation raises under any other
        hasher).
        Tickets already submitted keep the function they were queued with."""
        hasher = _hasher_id(hasher)
        self._check(self._lib.mirsha_ctx_set_hasher(self.ctx, hasher))

    @property
    def hasher(self) -> str:
        h = self._lib.mirsha_ctx_hasher(self.ctx)
        if h < 0:
            self._check(h)
        return {v: k for k, v in HASHERS.items()}[h]

    @property
    def sha512_pair_launches(self) -> int:
        """Launches of this engine that took the SHA-512/256 producer/consumer
        pair kernels (requests, lists and plan lists) since its creation
        (mirsha_ctx_sha512_pair_launches)."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.mirsha_ctx_sha512_pair_launches(self.ctx, ctypes.byref(n)))
        return n.value

    def set_timing(self, enable: bool) -> None:
        self._check(self._lib.mirsha_ctx_set_timing(self.ctx, 1 if enable else 0))

    def kernel_time(self, kernel: int) -> tuple[int, float]:
        n = ctypes.c_uint64(0)
        ms = ctypes.c_double(0.0)
        self._check(self._lib.mirsha_ctx_kernel_time(self.ctx, int(kernel), ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def set_timing_mask(self, kernels) -> None:
        """Time only these kernel ids (KERNEL_*) while timing is enabled."""
        m = 0
        for k in kernels:
            m |= 1 << int(k)
        self._check(self._lib.mirsha_ctx_set_timing_mask(self.ctx, m))

    def reset_timing(self) -> None:
        self._check(self._lib.mirsha_ctx_reset_timing(self.ctx))

    def sync(self) -> None:
        self._check(self._lib.mirsha_sync(self.ctx))

    # ------------------------------------------------------------ host API
    def hash_batch(self, arena, off: Sequence[int], length: Sequence[int], out=None) -> np.ndarray:
        """Digest of arena[off[i]:off[i]+len[i]] for every i (processor.go:133-143).
        out: optional reusable uint8 (n, 32) result array."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        if o.shape != ln.shape:
            raise ValueError("off and len differ in length")
        n = int(o.size)
        out = _out_rows(out, n)
        if n:
            self._check(self._lib.mirsha_hash_batch(self.ctx, _ptr(a), a.size, _ptr(o), _ptr(ln), n, _ptr(out)))
        return out

    def hash_messages(self, messages: Sequence[bytes]) -> np.ndarray:
        """One digest per message (each a single byte string)."""
        lens = np.fromiter((len(m) for m in messages), dtype=np.uint32, count=len(messages))
        off = np.zeros(len(messages), dtype=np.uint64)
        if len(messages) > 1:
            np.cumsum(lens[:-1], out=off[1:])
        arena = b"".join(messages)
        return self.hash_batch(arena, off, lens)

    def hash_slices(self, requests: Sequence[Sequence[bytes]], dedup: bool = False) -> np.ndarray:
        """Digest of concat(req) for each req = HashRequest.Data (actions.go:157-164).
        dedup=True hashes each distinct content once (mirsha_hash_slices_dedup);
        ``self.last_unique`` then holds the number of distinct requests."""
        sl = SliceArrays.from_requests(requests)
        return self.hash_slice_arrays(sl, dedup)

    def hash_slice_arrays(self, sl: "SliceArrays", dedup: bool = False) -> np.ndarray:
        """hash_slices over prepared slice arrays (pointer / length / first)."""
        n = sl.n
        out = np.empty((n, 32), dtype=np.uint8)
        if n == 0:
            self.last_unique = 0
            return out
        if dedup:
            u = ctypes.c_uint32(0)
            self._check(self._lib.mirsha_hash_slices_dedup(self.ctx, sl.ptr_p, sl.len_p, sl.first_p, n, _ptr(out),
                                                           ctypes.byref(u)))
            self.last_unique = u.value
        else:
            self._check(self._lib.mirsha_hash_slices(self.ctx, sl.ptr_p, sl.len_p, sl.first_p, n, _ptr(out)))
            self.last_unique = n
        return out

    def host_empty(self, nbytes: int) -> np.ndarray:
        """A uint8 array in page-locked host memory (mirsha_host_alloc), freed
        with the array: the caller's arena at PCIe rate."""
        p = ctypes.c_void_p()
        self._check(self._lib.mirsha_host_alloc(self.ctx, int(nbytes), ctypes.byref(p)))
        buf = (ctypes.c_uint8 * max(int(nbytes), 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=int(nbytes))
        import weakref

        weakref.finalize(buf, self._lib.mirsha_host_free, p.value)
        return arr

    def submit_slices(self, requests, dedup: bool = False) -> "Ticket":
        """Asynchronous, order-preserving submission (mirsha_submit_slices): the
        requests are packed before this returns; ``wait(ticket)`` yields the
        digests in origin order.  ``requests`` may be a list of slice lists or
        a SliceArrays."""
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        out = np.empty((sl.n, 32), dtype=np.uint8)
        t = ctypes.c_uint64(0)
        self._check(self._lib.mirsha_submit_slices(self.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, _ptr(out),
                                                   _lib.MIRSHA_SUBMIT_DEDUP if dedup else 0, ctypes.byref(t)))
        self._outstanding[t.value] = out
        # Submission t took the ring slot of t - ASYNC_SLOTS, which the library
        # completed (in order) before reusing it.
        self._retire(t.value - ASYNC_SLOTS)
        return Ticket(t.value, out)

    def submit_batch(self, arena, off, length, out=None) -> "Ticket":
        """Asynchronous arena submission (mirsha_submit_batch, the Go binding's
        chunked HashBatch): request i = arena[off[i]:off[i]+len[i]].  A
        page-locked arena (host_empty) is DMA'd from in place and must not
        change until the ticket is waited for; a page-locked ``out`` receives
        the digests by DMA."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        if o.shape != ln.shape:
            raise ValueError("off and len differ in length")
        n = int(o.size)
        out = _out_rows(out, n)
        t = ctypes.c_uint64(0)
        self._check(self._lib.mirsha_submit_batch(self.ctx, _ptr(a), a.size, _ptr(o), _ptr(ln), n, _ptr(out),
                                                  ctypes.byref(t)))
        self._outstanding[t.value] = (out, a)  # the arena too: it may be read until the ticket retires
        self._retire(t.value - ASYNC_SLOTS)
        return Ticket(t.value, out)

    def _expect_ticket(self, submit, n: int, expected, out, keep) -> "ExpectTicket":
        """One mirsha_submit_*_expect call (``submit(expect_of, rows, m, out,
        bits, count, ticket_ref)``) and its ticket."""
        expected = list(expected)
        if len(expected) != n:
            raise ValueError(f"{len(expected)} expectations for {n} requests")
        of, rows, short = expect_plan(expected)
        has = np.zeros(n, dtype=bool)
        has[of] = True
        out = _out_rows(out, n)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        count = np.zeros(1, dtype=np.uint32)
        t = ctypes.c_uint64(0)
        self._check(submit(_ptr(of), _ptr(rows), int(of.size), _ptr(out), _ptr(bits), count.ctypes.data,
                           ctypes.byref(t)))
        # everything the library may still read or write until the ticket retires
        self._outstanding[t.value] = (out, bits, count, of, rows, keep)
        self._retire(t.value - ASYNC_SLOTS)
        return ExpectTicket(t.value, out, has, bits, count, short)

    def submit_slices_expect_dedup(self, requests, expected, out=None) -> "ExpectTicket":
        """submit_slices_expect over a deduplicated cycle
        (mirsha_submit_slices_expect_dedup): equal requests are hashed once,
        with or without an expectation, and each is compared with its own
        expectation on the device.  ONE ring submission; the ticket, verdict
        and kept rows of submit_slices_expect, plus ``ticket.n_unique``."""
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        u = ctypes.c_uint32(0)
        ticket = self._expect_ticket(
            lambda of, rows, m, o, bits, count, t: self._lib.mirsha_submit_slices_expect_dedup(
                self.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, of, rows, m, o, bits, count, ctypes.byref(u), t),
            sl.n, expected, out, sl)
        ticket.n_unique = u.value
        return ticket

    @staticmethod
    def dedup_rows(requests) -> tuple[np.ndarray, int]:
        """The module's dedup_rows: the rows submit_slices_expect_dedup sends."""
        return dedup_rows(requests)

    def hash_slices_expect_dedup(self, requests, expected, out=None) -> "ExpectTicket":
        """submit_slices_expect_dedup + wait in one call
        (mirsha_hash_slices_expect_dedup): the retired ticket, ``mismatches``
        and ``n_unique`` set."""
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        u = ctypes.c_uint32(0)
        # the call hands no ticket out (it retired its own): value 0
        ticket = self._expect_ticket(
            lambda of, rows, m, o, bits, count, t: self._lib.mirsha_hash_slices_expect_dedup(
                self.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, of, rows, m, o, bits, count, ctypes.byref(u)),
            sl.n, expected, out, sl)
        self._outstanding.pop(ticket.value, None)
        ticket.n_unique = u.value
        ticket._resolve()
        return ticket

    def submit_slices_expect(self, requests, expected, out=None) -> "ExpectTicket":
        """submit_slices for a cycle whose requests may carry the digest their
        origin expects (mirsha_submit_slices_expect): ``expected[i]`` is None or
        request i's expectation.  ONE ring submission; the compare runs on the
        device behind the hashing kernel.  See ExpectTicket for what comes back."""
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        return self._expect_ticket(
            lambda of, rows, m, o, bits, count, t: self._lib.mirsha_submit_slices_expect(
                self.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, of, rows, m, o, bits, count, 0, t),
            sl.n, expected, out, sl)

    def submit_batch_expect(self, arena, off, length, expected, out=None) -> "ExpectTicket":
        """submit_batch with expectations (mirsha_submit_batch_expect): a
        page-locked, 16-byte aligned ``out`` receives the kept rows from the
        select kernel itself."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        if o.shape != ln.shape:
            raise ValueError("off and len differ in length")
        n = int(o.size)
        return self._expect_ticket(
            lambda of, rows, m, dst, bits, count, t: self._lib.mirsha_submit_batch_expect(
                self.ctx, _ptr(a), a.size, _ptr(o), _ptr(ln), n, of, rows, m, dst, bits, count, t),
            n, expected, out, a)

    def _retire(self, upto: int) -> None:
        for k in [k for k in self._outstanding if k <= upto]:
            del self._outstanding[k]

    def wait(self, ticket: "Ticket") -> np.ndarray:
        self._check(self._lib.mirsha_wait(self.ctx, ticket.value))
        self._retire(ticket.value)
        if isinstance(ticket, ExpectTicket):
            ticket._resolve()
        return ticket.out

    def poll(self, ticket: "Ticket") -> bool:
        done = ctypes.c_int(0)
        self._check(self._lib.mirsha_poll(self.ctx, ticket.value, ctypes.byref(done)))
        if done.value:
            self._retire(ticket.value)
            if isinstance(ticket, ExpectTicket):
                ticket._resolve()
        return bool(done.value)

    def hash_requests_then_batches(self, arena, off, length, idx, batch_first, out=None, batch_out=None):
        """Request digests, then batch digests over them on device (sequence.go:154-157).

        out / batch_out: optional C-contiguous uint8 (n, 32) / (n_batches, 32)
        arrays reused across calls.  A fresh 32 MiB result array costs ~30 ms
        of first-touch page faults per call (glibc hands large allocations
        out as new mmaps), which is more than the GPU work at 1M requests."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        fs = np.ascontiguousarray(batch_first, dtype=np.uint32)
        n, nb = int(o.size), int(fs.size) - 1
        if nb < 0:
            raise ValueError("batch_first needs n_batches + 1 entries")
        req = _out_rows(out, n)
        bat = _out_rows(batch_out, nb)
        self._check(
            self._lib.mirsha_hash_requests_then_batches(
                self.ctx, _ptr(a), a.size, _ptr(o), _ptr(ln), n, _ptr(ix), _ptr(fs), nb, _ptr(req), _ptr(bat)
            )
        )
        return req, bat

    def digest_lists(self, digests, idx, list_first) -> np.ndarray:
        """SHA-256 over ordered lists of 32-byte digests (batch / VerifyBatch / checkpoint chain)."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        fs = np.ascontiguousarray(list_first, dtype=np.uint32)
        nl = int(fs.size) - 1
        out = np.empty((max(nl, 0), 32), dtype=np.uint8)
        if nl > 0:
            self._check(
                self._lib.mirsha_digest_lists(self.ctx, _ptr(d), d.shape[0], _ptr(ix), _ptr(fs), nl, _ptr(out))
            )
        return out

    # ------------------------------------------------- verify on the device
    def _verdict(self, call, n: int, expected) -> np.ndarray:
        """Runs one mirsha_verify_* call (``call(expected_ptr, bits_ptr, count_ref)``)
        and returns the sorted mismatching indices, host-side length mismatches included."""
        exp, short = _expected_rows(expected, n)
        if n == 0:
            return np.empty(0, dtype=np.int64)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        count = ctypes.c_uint32(0)
        self._check(call(_ptr(exp), _ptr(bits), ctypes.byref(count)))
        bad = mismatch_indices(bits, n)
        if bad.size != count.value:
            raise MirshaError(_lib.MIRSHA_EHIP, f"verify: bitmap has {bad.size} bits set, count is {count.value}")
        return np.union1d(bad, short) if short.size else bad

    def verify_slices(self, requests, expected) -> np.ndarray:
        """Hash each request (as hash_slices) and compare with expected[i] on the
        device (VerifyRequest, state_machine.go:408-417): the sorted indices
        whose digest differs.  ``expected``: (n, 32) uint8 array or a sequence
        of bytes (an entry that is not 32 bytes long is a mismatch).  Only the
        verdict (a bitmap and a count) comes back from the device."""
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        return self._verdict(lambda e, b, c: self._lib.mirsha_verify_slices(
            self.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, e, b, c), sl.n, expected)

    def verify_batch(self, arena, off: Sequence[int], length: Sequence[int], expected) -> np.ndarray:
        """verify_slices over requests packed in one arena (hash_batch's arguments)."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        if o.shape != ln.shape:
            raise ValueError("off and len differ in length")
        n = int(o.size)
        return self._verdict(lambda e, b, c: self._lib.mirsha_verify_batch(
            self.ctx, _ptr(a), a.size, _ptr(o), _ptr(ln), n, e, b, c), n, expected)

    def verify_digest_lists(self, digests, idx, list_first, expected) -> np.ndarray:
        """digest_lists with one expected digest per list, compared on the device
        (VerifyBatch, batch_tracker.go:139-174): the sorted mismatching list indices."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        fs = np.ascontiguousarray(list_first, dtype=np.uint32)
        nl = int(fs.size) - 1
        if nl < 0:
            raise ValueError("list_first needs n_lists + 1 entries")
        return self._verdict(lambda e, b, c: self._lib.mirsha_verify_digest_lists(
            self.ctx, _ptr(d), d.shape[0], _ptr(ix), _ptr(fs), nl, e, b, c), nl, expected)

    # ---------------------------------------------------------- device API
    def verify_digests_device(self, d_digests: int, d_expected: int, n: int, d_bits: int, d_count: int) -> None:
        """Compare n device digests with n expected ones (mirsha_verify_digests_device):
        mismatch bitmap (ceil(n/64) uint64 words) to d_bits, count (uint32) to
        d_count; asynchronous on the engine's stream."""
        self._check(self._lib.mirsha_verify_digests_device(self.ctx, d_digests or None, d_expected or None, int(n),
                                                           d_bits or None, d_count or None))

    def hash_batch_device(self, d_arena: int, arena_len: int, d_off: int, d_len: int, d_order: int | None,
                          n: int, d_out: int) -> None:
        self._check(self._lib.mirsha_hash_batch_device(self.ctx, d_arena, arena_len, d_off, d_len, d_order, n, d_out))

    def bucket_order_device(self, d_len: int, n: int, min_len: int, max_len: int, d_order: int) -> bool:
        """The bucket order of n device-resident lengths into d_order (u32[n]),
        built on the device, asynchronous on the engine's stream
        (mirsha_bucket_order_device).  min_len / max_len bound the lengths.
        True when the order is the identity (one block count): d_order holds it,
        and None may be passed downstream instead."""
        rc = self._lib.mirsha_bucket_order_device(self.ctx, d_len or None, int(n), int(min_len), int(max_len),
                                                  d_order or None)
        if rc < 0:
            self._check(rc)
        return rc == 1

    def offsets_device(self, d_len: int, n: int, d_off: int) -> None:
        """d_off (u64[n]) = exclusive scan of d_len (u32[n]), on the device,
        asynchronous on the engine's stream (mirsha_offsets_device)."""
        self._check(self._lib.mirsha_offsets_device(self.ctx, d_len or None, int(n), d_off or None))

    def digest_lists_device(self, d_digests: int, n_digests: int, d_idx: int, d_first: int, n_lists: int,
                            n_entries: int, d_out: int) -> None:
        self._check(self._lib.mirsha_digest_lists_device(self.ctx, d_digests, n_digests, d_idx, d_first, n_lists,
                                                         n_entries, d_out))

    def pipeline(self, n_req: int, idx, list_first, length=None, mode: int | str | None = None,
                 hasher: str | int | None = None) -> "Pipeline":
        """Plan for request -> batch-digest runs with this list shape (host index lists).
        mode: PIPELINE_AUTO (default) / _FUSED / _SEQUENTIAL or its name.
        hasher: "sha256" / "sha512_256" or its id: the plan hashes with it,
        whatever the engine's hasher is now (mirsha_pipeline_create_hasher;
        mode None = AUTO; under "sha512_256" a plan is sequential, "fused"
        raises), and runs only while the engine hashes with the same one.
        None: a SHA-256 plan by mirsha_pipeline_create / _create_mode."""
        return Pipeline(self, n_req, idx, list_first, length, mode, hasher)

    def hash_requests_then_batches_device(self, plan: "Pipeline", d_arena: int, arena_len: int, d_off: int,
                                          d_len: int, d_req_out: int, d_batch_out: int) -> None:
        self._check(self._lib.mirsha_hash_requests_then_batches_device(
            self.ctx, plan.handle, d_arena, arena_len, d_off, d_len, d_req_out, d_batch_out))

    def pipeline_overlap_device(self, plan: "Pipeline", d_arena: int, arena_len: int, d_off: int, d_len: int,
                                d_req_out: int, d_prev_req: int, d_prev_batch_out: int) -> None:
        """One launch: this cycle's requests -> d_req_out and the previous cycle's
        batch digests from d_prev_req -> d_prev_batch_out (0 = none; see mirsha.h)."""
        self._check(self._lib.mirsha_pipeline_overlap_device(
            self.ctx, plan.handle, d_arena or None, arena_len, d_off or None, d_len or None, d_req_out or None,
            d_prev_req or None, d_prev_batch_out or None))

    def synth_requests_device(self, seed: int, first: int, count: int, data_len: int, d_arena: int) -> None:
        self._check(self._lib.mirsha_synth_requests_device(self.ctx, seed, first, count, data_len, d_arena))

    def synth_mixed_lengths_device(self, seed: int, first: int, count: int, d_len: int) -> None:
        """Config-5 message lengths (u32) of requests [first, first + count) into d_len."""
        self._check(self._lib.mirsha_synth_mixed_lengths_device(self.ctx, seed, first, count, d_len))

    def synth_mixed_device(self, seed: int, first: int, count: int, d_off: int, d_arena: int) -> None:
        """Config-5 message bytes of requests [first, first + count) at d_arena + d_off[r]."""
        self._check(self._lib.mirsha_synth_mixed_device(self.ctx, seed, first, count, d_off, d_arena))

    HOST_PHASES = ("validate", "plan", "pack", "device", "scatter", "total", "chunks")

    def host_profile(self) -> dict:
        """Host-side phases (ms) of the last slice submission (mirsha_ctx_host_profile)."""
        buf = (ctypes.c_double * len(self.HOST_PHASES))()
        n = self._lib.mirsha_ctx_host_profile(self.ctx, buf, len(self.HOST_PHASES))
        if n < 0:
            self._check(n)
        return {k: buf[i] for i, k in enumerate(self.HOST_PHASES)}

    def clock_probe(self, iters: int = 128) -> tuple[float, float]:
        """(clock GHz held under the compression load, SIMD cycles per 64-lane
        compression with no memory traffic): mirsha_clock_probe."""
        ghz, cyc = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self._lib.mirsha_clock_probe(self.ctx, int(iters), ctypes.byref(ghz), ctypes.byref(cyc)))
        return ghz.value, cyc.value


class Pipeline:
    """mirsha_pipeline: a request -> batch-digest plan reused across runs of one
    shape (see include/mirsha.h for the modes)."""

    def __init__(self, engine: Engine, n_req: int, idx, list_first, length=None, mode=None, hasher=None):
        self._lib = engine._lib
        self._engine = engine
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        fs = np.ascontiguousarray(list_first, dtype=np.uint32)
        ln = None if length is None else np.ascontiguousarray(length, dtype=np.uint32)
        h = ctypes.c_void_p()
        if hasher is not None:
            # (an unknown id goes to the library, whose refusal names it)
            hid = _hasher_id(hasher) if isinstance(hasher, str) else int(hasher)
            m = PIPELINE_AUTO if mode is None else PIPELINE_MODES[mode] if isinstance(mode, str) else int(mode)
            engine._check(self._lib.mirsha_pipeline_create_hasher(engine.ctx, int(n_req), _ptr(ln), _ptr(ix),
                                                                  _ptr(fs), int(fs.size) - 1, m, hid, ctypes.byref(h)))
        elif mode is None:
            engine._check(self._lib.mirsha_pipeline_create(engine.ctx, int(n_req), _ptr(ln), _ptr(ix), _ptr(fs),
                                                           int(fs.size) - 1, ctypes.byref(h)))
        else:
            m = PIPELINE_MODES[mode] if isinstance(mode, str) else int(mode)
            engine._check(self._lib.mirsha_pipeline_create_mode(engine.ctx, int(n_req), _ptr(ln), _ptr(ix),
                                                                _ptr(fs), int(fs.size) - 1, m, ctypes.byref(h)))
        self.handle = h
        self.mode = int(self._lib.mirsha_pipeline_mode(h))
        # 1: a fused plan built sequential after its placement probe (mirsha_pipeline_fallback)
        self.fallback = int(self._lib.mirsha_pipeline_fallback(h)) if hasattr(self._lib, "mirsha_pipeline_fallback") \
            else 0
        self.n_req = int(n_req)
        self.n_lists = int(fs.size) - 1

    @property
    def mode_name(self) -> str:
        return {v: k for k, v in PIPELINE_MODES.items()}[self.mode]

    @property
    def hasher(self) -> str:
        """The name of the plan's hash function (mirsha_pipeline_hasher)."""
        h = self._lib.mirsha_pipeline_hasher(self.handle)
        if h < 0:
            check(h)
        return {v: k for k, v in HASHERS.items()}[h]

    def status(self) -> None:
        """Synchronise and raise if a fused run's readiness watchdog expired."""
        self._engine._check(self._lib.mirsha_pipeline_status(self._engine.ctx, self.handle))

    def shape(self) -> tuple[int, int, int]:
        """(n_tiles, n_counters, n_groups) of a fused plan."""
        t, c, g = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(self._lib.mirsha_pipeline_shape(self.handle, ctypes.byref(t), ctypes.byref(c), ctypes.byref(g)))
        return t.value, c.value, g.value

    def split_tiles(self) -> tuple[int, int]:
        """(split tiles, segments per tile) of a fused plan (mirsha_pipeline_split_tiles)."""
        n, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(self._lib.mirsha_pipeline_split_tiles(self.handle, ctypes.byref(n), ctypes.byref(k)))
        return n.value, k.value

    def trace(self) -> np.ndarray | None:
        """Last run's fused timeline (MIRSHA_FUSED_TRACE=1 at plan creation), see include/mirsha.h."""
        n = ctypes.c_uint64(0)
        self._engine._check(self._lib.mirsha_pipeline_trace(self._engine.ctx, self.handle, None, 0, ctypes.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value, dtype=np.uint64)
        self._engine._check(self._lib.mirsha_pipeline_trace(self._engine.ctx, self.handle, _ptr(out), n.value,
                                                            ctypes.byref(n)))
        return out

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.mirsha_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StateObject:
    """What CheckpointChains and HashStreams share: hash states on the device
    (``handle``, of ``_engine``) whose programmes run in one call or as a
    ValuesTicket of the engine's ring."""

    _VALUES = ("", "")  # the count check's message: the call, what yields a value
    _DESTROY = ""

    def _values(self, call, args, n: int, out=None, keep=None, ticket=None):
        """call(ctx, handle, *args, out, &count[, &ticket]) for a programme with
        ``n`` value ops, and the count check.  Without ``ticket`` (a
        ValuesTicket class) the call is synchronous and the (n, 32) values are
        returned; with it the ticket is, and until it retires it keeps
        ``out``, ``keep`` and this object (the kernel writes its state)."""
        out = _out_rows(out, n)
        k, t = ctypes.c_uint32(0), ctypes.c_uint64(0)
        eng = self._engine
        eng._check(call(eng.ctx, self.handle, *args, _ptr(out), ctypes.byref(k), *([ctypes.byref(t)] if ticket else [])))
        if k.value != n:
            raise MirshaError(_lib.MIRSHA_EHIP, f"{self._VALUES[0]}: {k.value} values for {n} {self._VALUES[1]}")
        if ticket is None:
            return out
        eng._outstanding[t.value] = (out, keep, self)
        eng._retire(t.value - ASYNC_SLOTS)
        return ticket(t.value, out)

    def close(self) -> None:
        if getattr(self, "handle", None):
            getattr(self._lib, self._DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CheckpointChains(_StateObject):
    """Streaming checkpoint chains on the device (mirsha_chains_*): one running
    hash per application node, as testengine's NodeState.ActiveHash
    (testengine/recorder.go:186-256).  write() = ActiveHash.Write of committed
    request digests, sum() = ActiveHash.Sum(nil) (state unchanged),
    reset() = NodeState.Set's fresh hasher.

    The chains hash with ``hasher`` ("sha256" or "sha512_256"), fixed here;
    ``None`` takes the engine's hasher as it is now.  Every call but reset()
    raises MirshaError (MIRSHA_EINVAL) while the engine hashes with another
    function: a log that hashes differently from the requests is a
    misconfiguration."""

    _VALUES, _DESTROY = ("commit", "checkpoints"), "mirsha_chains_destroy"

    def __init__(self, engine: Engine, n_chains: int, hasher: str | int | None = None):
        self._engine = engine
        self._lib = engine._lib
        hid = _hasher_id(engine.hasher if hasher is None else hasher)
        h = ctypes.c_void_p()
        engine._check(self._lib.mirsha_chains_create_hasher(engine.ctx, int(n_chains), hid, ctypes.byref(h)))
        self.handle = h
        self.n = int(n_chains)

    @property
    def hasher(self) -> str:
        h = self._lib.mirsha_chains_hasher(self.handle)
        if h < 0:
            self._engine._check(h)
        return {v: k for k, v in HASHERS.items()}[h]

    @property
    def pair_launches(self) -> int:
        """Commit launches of these chains (write, the commit calls and the
        commit tickets) that took the SHA-512/256 producer/consumer pair
        kernels, counted where they are queued (mirsha_chains_pair_launches).
        Always 0 for "sha256" chains."""
        n = ctypes.c_uint64(0)
        self._engine._check(self._lib.mirsha_chains_pair_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def write(self, digests, chain_of) -> None:
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        c = np.ascontiguousarray(chain_of, dtype=np.uint32).reshape(-1)
        if c.size != d.shape[0]:
            raise ValueError("one chain id per digest")
        if c.size:
            self._engine._check(self._lib.mirsha_chains_absorb(self._engine.ctx, self.handle, _ptr(d), _ptr(c),
                                                               c.size))

    def sum(self, which) -> np.ndarray:
        w = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        out = np.empty((w.size, 32), dtype=np.uint8)
        if w.size:
            self._engine._check(self._lib.mirsha_chains_sum(self._engine.ctx, self.handle, _ptr(w), w.size,
                                                            _ptr(out)))
        return out

    def reset(self, which) -> None:
        w = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        if w.size:
            self._engine._check(self._lib.mirsha_chains_reset(self._engine.ctx, self.handle, _ptr(w), w.size))

    def commit(self, digests, op_chain, op_digest, out=None) -> np.ndarray:
        """One cycle's commit programme in ONE call (mirsha_chains_commit, the
        commit loop of processor.go:145-168): op i acts on chain op_chain[i];
        op_digest[i] is a row of ``digests`` to write, MIRSHA_NULL_INDEX (a
        null request: nothing) or MIRSHA_COMMIT_CHECKPOINT (Sum, then a fresh
        hasher).  Returns the checkpoint values, (k, 32) uint8, in op order
        (in ``out`` when one is given)."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        return self._commit(self._lib.mirsha_chains_commit, _ptr(d), d.shape[0], op_chain, op_digest, out)

    def commit_device(self, d_digests: int, n_digests: int, op_chain, op_digest, out=None) -> np.ndarray:
        """commit() with the digest table in device memory (a raw device
        address, 16-byte aligned; e.g. the output of ``hash_batch_device``).
        The ops stay host arrays and the values come back to the host."""
        return self._commit(self._lib.mirsha_chains_commit_device, int(d_digests) or None, int(n_digests), op_chain,
                            op_digest, out)

    def _commit(self, call, table, n_digests: int, op_chain, op_digest, *ring):
        """``ring``: (out, keep, CommitTicket) of a submission."""
        oc, od = _commit_ops(op_chain, op_digest)
        return self._values(call, (table, n_digests, _ptr(oc), _ptr(od), oc.size),
                            int(np.count_nonzero(od == _lib.MIRSHA_COMMIT_CHECKPOINT)), *ring)

    def submit_commit(self, digests, op_chain, op_digest, out=None) -> "CommitTicket":
        """commit() as a submission of the engine's ring
        (mirsha_chains_commit_submit): the programme is checked, planned and
        copied before this returns, the device runs it on the engine's commit
        stream beside whatever hashing is queued, and ``engine.wait(ticket)``
        returns the checkpoint values, (k, 32) uint8 in op order.  Tickets
        retire in submission order, mixed with the hashing tickets.  A
        page-locked ``out`` (``engine.host_empty``) receives the values from
        the kernel itself."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        return self._commit(self._lib.mirsha_chains_commit_submit, _ptr(d), d.shape[0], op_chain, op_digest, out,
                            None, CommitTicket)

    def submit_commit_device(self, d_digests: int, n_digests: int, op_chain, op_digest, out=None,
                             keep=None) -> "CommitTicket":
        """submit_commit() with the digest table in device memory (a raw device
        address, 16-byte aligned): it is read behind whatever is queued on the
        engine's stream at this moment, e.g. the ``hash_batch_device`` that
        writes it, and must stay intact until the ticket retires (``keep``:
        an object to hold on to until then)."""
        return self._commit(self._lib.mirsha_chains_commit_submit_device, int(d_digests) or None, int(n_digests),
                            op_chain, op_digest, out, keep, CommitTicket)


def _stream_ops(ops) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """A stream programme as the four op arrays of mirsha_streams_run: either
    those arrays themselves, ``(op_stream, op_kind, op_off, op_len)``, or a
    sequence of ``(stream, STREAM_WRITE, off, len)`` / ``(stream, kind)`` tuples."""
    if isinstance(ops, tuple) and len(ops) == 4 and all(isinstance(a, np.ndarray) for a in ops):
        cols = ops
    else:
        rows = [tuple(op) + (0, 0) * (len(op) == 2) for op in ops]
        if any(len(r) != 4 for r in rows):
            raise ValueError("an op is (stream, kind) or (stream, kind, off, len)")
        cols = tuple(zip(*rows)) if rows else ((), (), (), ())
    os_, ok, oo, ol = (np.ascontiguousarray(c, dtype=t).reshape(-1)
                       for c, t in zip(cols, (np.uint32, np.uint32, np.uint64, np.uint32)))
    if not os_.size == ok.size == oo.size == ol.size:
        raise ValueError("one stream, kind, offset and length per op")
    return os_, ok, oo, ol


def stream_plan(ops, n_streams: int, arena_len: int, pack: bool = False):
    """Host-only mirsha_stream_plan: the arrays ``HashStreams.run`` (pack=True)
    / ``run_device`` (pack=False) send to the device.  Returns (act, efirst,
    ent_kind, ent_off, ent_len, n_values, n_bytes): the active streams
    (ascending), their entry ranges in op order with zero-length writes
    dropped, per entry the kind in bits 0-1 (and, for a sum, the values row
    above them), the write's offset and length, the number of sums and the
    bytes the writes name.  pack=True: offsets into the packed bytes -- every
    distinct (off, len) range once, in the order of its first entry, without
    gaps -- and their size as n_bytes."""
    os_, ok, oo, ol = _stream_ops(ops)
    cap = min(os_.size, int(n_streams))
    act = np.zeros(cap, dtype=np.uint32)
    efirst = np.zeros(cap + 1, dtype=np.uint32)
    kind = np.zeros(os_.size, dtype=np.uint32)
    off = np.zeros(os_.size, dtype=np.uint64)
    ln = np.zeros(os_.size, dtype=np.uint32)
    na, ne, nv, bad = (ctypes.c_uint32(0) for _ in range(4))
    nb = ctypes.c_uint64(0)
    rc = _lib.load().mirsha_stream_plan(_ptr(os_), _ptr(ok), _ptr(oo), _ptr(ol), os_.size, int(n_streams),
                                        int(arena_len), 1 if pack else 0, _ptr(act), efirst.ctypes.data, _ptr(kind),
                                        _ptr(off), _ptr(ln), ctypes.byref(na), ctypes.byref(ne), ctypes.byref(nv),
                                        ctypes.byref(nb), ctypes.byref(bad))
    if rc != _lib.MIRSHA_OK:
        err = MirshaError(rc, f"stream plan: op {bad.value}" if bad.value != 0xFFFFFFFF else "stream plan: arguments")
        err.bad_op = None if bad.value == 0xFFFFFFFF else bad.value
        raise err
    return (act[:na.value], efirst[:na.value + 1], kind[:ne.value], off[:ne.value], ln[:ne.value], nv.value,
            nb.value)


def stream_seg_plan(ops, n_streams: int, arena_len: int, pack: bool = False):
    """Host-only mirsha_stream_seg_plan: ``stream_plan``'s per-stream programmes
    cut after every STREAM_SUM_RESET and STREAM_RESET entry, one segment per
    lane of the ring form (``HashStreams.submit``).  Returns (seg_stream,
    sfirst, seg_flags, ent_kind, ent_off, ent_len, n_values, n_bytes, n_active):
    segment s belongs to stream ``seg_stream[s]`` and runs entries
    ``sfirst[s]:sfirst[s+1]`` of the entry arrays (stream_plan's, unchanged);
    ``seg_flags[s]`` has MIRSHA_STREAM_SEG_FIRST on the stream's first segment
    (it starts from the stored state, every other one from Hasher()) and
    MIRSHA_STREAM_SEG_LAST on the one holding the stream's final entry."""
    os_, ok, oo, ol = _stream_ops(ops)
    seg_stream = np.zeros(os_.size, dtype=np.uint32)
    sfirst = np.zeros(os_.size + 1, dtype=np.uint32)
    seg_flags = np.zeros(os_.size, dtype=np.uint32)
    kind = np.zeros(os_.size, dtype=np.uint32)
    off = np.zeros(os_.size, dtype=np.uint64)
    ln = np.zeros(os_.size, dtype=np.uint32)
    ns, na, ne, nv, bad = (ctypes.c_uint32(0) for _ in range(5))
    nb = ctypes.c_uint64(0)
    rc = _lib.load().mirsha_stream_seg_plan(_ptr(os_), _ptr(ok), _ptr(oo), _ptr(ol), os_.size, int(n_streams),
                                            int(arena_len), 1 if pack else 0, _ptr(seg_stream), sfirst.ctypes.data,
                                            _ptr(seg_flags), _ptr(kind), _ptr(off), _ptr(ln), ctypes.byref(ns),
                                            ctypes.byref(na), ctypes.byref(ne), ctypes.byref(nv), ctypes.byref(nb),
                                            ctypes.byref(bad))
    if rc != _lib.MIRSHA_OK:
        err = MirshaError(rc, f"stream segment plan: op {bad.value}" if bad.value != 0xFFFFFFFF
                          else "stream segment plan: arguments")
        err.bad_op = None if bad.value == 0xFFFFFFFF else bad.value
        raise err
    return (seg_stream[:ns.value], sfirst[:ns.value + 1], seg_flags[:ns.value], kind[:ne.value], off[:ne.value],
            ln[:ne.value], nv.value, nb.value, na.value)


def stream_state_bytes(hasher: str | int) -> int:
    """Bytes of one exported stream state under a hasher: 108 for "sha256",
    204 for "sha512_256" (mirsha_stream_state_bytes; host only)."""
    n = ctypes.c_uint32(0)
    check(_lib.load().mirsha_stream_state_bytes(_hasher_id(hasher), ctypes.byref(n)))
    return n.value


class _StreamsHasher(str):
    """``HashStreams.hasher``: the name of the streams' hash function, and,
    called, a new hash.Hash-shaped object on a free stream (the method it was
    before the streams had a hasher of their own)."""

    def __new__(cls, name: str, streams: "HashStreams"):
        self = super().__new__(cls, name)
        self._streams = streams
        return self

    def __call__(self) -> "StreamHasher":
        return self._streams._new_hasher()


class HashStreams(_StateObject):
    """Streaming hash states on the device (mirsha_streams_*): n hashers in
    the reference's own shape, ``type Hasher func() hash.Hash``
    (processor.go:21) -- Write any bytes any number of times, Sum at any point
    without disturbing the state, Reset -- whose midstate, unfinished block and
    length stay on the device across calls.  ``run`` is ONE programme over any
    number of streams in ONE launch; ``hasher()`` / ``flush`` is the hash.Hash
    form on top of it.  ``submit`` / ``submit_device`` / ``submit_flush`` are
    the same as tickets of the engine's ring (one lane per stretch between
    resets, beside the hashing).  ``bytes_sent`` counts the bytes of the
    distinct ranges the write ops of each ``run`` / ``submit`` named (what
    crossed PCIe); ``runs`` the calls.

    The streams hash with ``hasher`` ("sha256" or "sha512_256"), fixed here;
    ``None`` takes the engine's hasher as it is now.  Every call that runs,
    submits, exports or imports raises MirshaError (MIRSHA_EINVAL) while the
    engine hashes with another function.  ``.hasher`` is that name; called,
    ``.hasher()``, it gives a hash.Hash-shaped object on a free stream."""

    _VALUES, _DESTROY = ("streams", "sums"), "mirsha_streams_destroy"

    def __init__(self, engine: Engine, n_streams: int, hasher: str | int | None = None):
        self._engine = engine
        self._lib = engine._lib
        hid = _hasher_id(engine.hasher if hasher is None else hasher)
        h = ctypes.c_void_p()
        engine._check(self._lib.mirsha_streams_create_hasher(engine.ctx, int(n_streams), hid, ctypes.byref(h)))
        self.handle = h
        self._hasher_name = {v: k for k, v in HASHERS.items()}[hid]
        self.state_bytes = stream_state_bytes(hid)
        self.digest_size, self.block_size = hasher_info(hid)
        self.n = int(n_streams)
        self.bytes_sent = 0
        self.runs = 0
        self._free = list(range(self.n - 1, -1, -1))

    def run(self, ops, arena=b"") -> np.ndarray:
        """Runs the programme ``ops`` (see ``_stream_ops``) over host bytes:
        a write op names ``arena[off:off+len]``.  Returns the (k, 32) uint8
        digests of its k STREAM_SUM / STREAM_SUM_RESET ops, in op order."""
        a = _as_u8(arena)
        return self._run(self._lib.mirsha_streams_run, _ptr(a), a.size, ops)

    def run_device(self, ops, d_arena: int, arena_len: int) -> np.ndarray:
        """run() with the arena in device memory (a raw device address, any
        alignment), read where it lies behind whatever is queued on the
        engine's stream."""
        return self._run(self._lib.mirsha_streams_run_device, int(d_arena) or None, int(arena_len), ops)

    def _run(self, call, arena, arena_len: int, ops, *ring):
        """``ring``: (out, keep, StreamTicket) of a submission."""
        os_, ok, oo, ol = _stream_ops(ops)
        sums = (ok == _lib.MIRSHA_STREAM_SUM) | (ok == _lib.MIRSHA_STREAM_SUM_RESET)
        got = self._values(call, (arena, arena_len, _ptr(os_), _ptr(ok), _ptr(oo), _ptr(ol), os_.size),
                           int(np.count_nonzero(sums)), *ring)
        self._count(call in (self._lib.mirsha_streams_run, self._lib.mirsha_streams_submit), ok, oo, ol)
        return got

    def _count(self, host: bool, ok, oo, ol) -> None:
        if host:  # every distinct (off, len) range once: a sort and a compare with the neighbour
            w = (ok == _lib.MIRSHA_STREAM_WRITE) & (ol != 0)
            off, ln = oo[w], ol[w]
            order = np.lexsort((ln, off))
            off, ln = off[order], ln[order]
            again = (off[1:] == off[:-1]) & (ln[1:] == ln[:-1])
            self.bytes_sent += int(ln.sum(dtype=np.uint64)) - int(ln[1:][again].sum(dtype=np.uint64))
        self.runs += 1

    def submit(self, ops, arena=b"", out=None) -> "StreamTicket":
        """run() as a submission of the engine's ring (mirsha_streams_submit):
        the programme is checked, planned and copied (ops and written bytes)
        before this returns, the device runs it on the engine's commit stream
        beside whatever hashing is queued, one lane per stretch between
        Sum-then-Reset / Reset ops, and ``engine.wait(ticket)`` returns the
        digests, (k, 32) uint8 in op order.  Tickets retire in submission
        order, mixed with the hashing and commit tickets.  A page-locked
        ``out`` (``engine.host_empty``) receives the values from the kernel
        itself."""
        a = _as_u8(arena)
        return self._run(self._lib.mirsha_streams_submit, _ptr(a), a.size, ops, out, None, StreamTicket)

    def submit_device(self, ops, d_arena: int, arena_len: int, out=None, keep=None) -> "StreamTicket":
        """submit() with the arena in device memory (a raw device address, any
        alignment): it is read behind whatever is queued on the engine's
        stream at this moment, e.g. the ``hash_batch_device`` that writes it,
        and must stay intact until the ticket retires (``keep``: an object to
        hold on to until then)."""
        return self._run(self._lib.mirsha_streams_submit_device, int(d_arena) or None, int(arena_len), ops, out,
                         keep, StreamTicket)

    def export_state(self, which) -> np.ndarray:
        """The states of streams ``which`` as (k, ``state_bytes``) uint8 rows in
        the layout of Go 1.14's MarshalBinary: crypto/sha256's (108 bytes) or,
        for SHA-512/256 streams, crypto/sha512's (204) (mirsha_streams_export)."""
        w = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        out = np.empty((w.size, self.state_bytes), dtype=np.uint8)
        if w.size:
            self._engine._check(self._lib.mirsha_streams_export(self._engine.ctx, self.handle, _ptr(w), w.size,
                                                                _ptr(out)))
        return out

    def import_state(self, which, states) -> None:
        """Sets streams ``which`` from such rows (mirsha_streams_import); a row
        that does not begin with the magic is refused and nothing changes."""
        w = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        if isinstance(states, (bytes, bytearray, memoryview)):
            states = np.frombuffer(bytes(states), dtype=np.uint8)
        rows = np.ascontiguousarray(states, dtype=np.uint8).reshape(-1, self.state_bytes)
        if rows.shape[0] != w.size:
            raise ValueError(f"one {self.state_bytes}-byte state per stream")
        if w.size:
            self._engine._check(self._lib.mirsha_streams_import(self._engine.ctx, self.handle, _ptr(w), w.size,
                                                                _ptr(rows)))

    # ------------------------------------------------------- hash.Hash form
    @property
    def hasher(self) -> "_StreamsHasher":
        """The streams' hash function, "sha256" or "sha512_256"; called,
        ``hasher()``, a hash.Hash-shaped object bound to a free stream
        (``close()`` gives the stream back).  Its first flush starts with a
        Reset, so it is Hasher() whatever the stream held."""
        return _StreamsHasher(self._hasher_name, self)

    def _new_hasher(self) -> "StreamHasher":
        if not self._free:
            raise MirshaError(_lib.MIRSHA_ERANGE, f"all {self.n} streams are in use")
        return StreamHasher(self, self._free.pop())

    def flush(self, hashers, sums: bool = True) -> list:
        """Sends the pending Resets and writes of ``hashers`` -- and with
        ``sums`` one Sum each -- in ONE ``run``: the batched use.  Returns the
        digests (bytes) in the order of ``hashers``, or [] without sums."""
        ops, arena = self._flush_programme(hashers, sums)
        out = self.run(ops, arena) if ops else np.empty((0, 32), dtype=np.uint8)
        for hs in hashers:  # sent: only now, a refused run leaves them pending
            hs._pending, hs._reset = [], False
        return [row.tobytes() for row in out]

    def submit_flush(self, hashers, sums: bool = True) -> "StreamTicket":
        """flush() as ONE ``submit``: the hashers are marked sent when this
        returns (a refused submission leaves them pending), and
        ``engine.wait(ticket)`` gives the digests, one row per hasher in the
        order of ``hashers`` ((0, 32) without sums)."""
        ops, arena = self._flush_programme(hashers, sums)
        ticket = self.submit(ops, arena)
        for hs in hashers:
            hs._pending, hs._reset = [], False
        return ticket

    def _flush_programme(self, hashers, sums: bool):
        """(ops, arena) of the pending Resets and writes of ``hashers``."""
        ops, parts, at = [], [], 0
        for hs in hashers:
            if hs._streams is not self or hs.stream is None:
                raise ValueError("a hasher of another HashStreams, or a closed one")
            if hs._reset:
                ops.append((hs.stream, _lib.MIRSHA_STREAM_RESET, 0, 0))
            size = sum(len(p) for p in hs._pending)
            if size:
                ops.append((hs.stream, _lib.MIRSHA_STREAM_WRITE, at, size))
                parts.extend(hs._pending)
                at += size
            if sums:
                ops.append((hs.stream, _lib.MIRSHA_STREAM_SUM, 0, 0))
        return ops, b"".join(parts)


class StreamHasher:
    """hash.Hash (Write / Sum / Reset / Size / BlockSize) over one stream of a
    ``HashStreams``: ``write`` buffers on the host, ``sum`` sends only the
    bytes not sent yet plus a Sum (the state stays on the device, so a hasher
    summed after every write sends each byte once), ``reset`` is sent with the
    next flush.  ``size`` / ``block_size`` are Go's Size() / BlockSize() of the
    streams' hasher: 32 / 64 under SHA-256, 32 / 128 under SHA-512/256."""

    def __init__(self, streams: HashStreams, stream: int):
        self._streams = streams
        self.size, self.block_size = streams.digest_size, streams.block_size
        self.stream = stream
        self._pending: list[bytes] = []
        self._reset = True

    def write(self, data) -> int:
        if self.stream is None:
            raise ValueError("write to a closed hasher")
        if len(data):
            self._pending.append(bytes(data))
        return len(data)

    def sum(self, b: bytes = b"") -> bytes:
        return bytes(b) + self._streams.flush([self])[0]

    def reset(self) -> None:
        self._pending, self._reset = [], True

    def close(self) -> None:
        if self.stream is not None:
            self._streams._free.append(self.stream)
            self.stream = None
            self._pending = []


def bucket_order(length: Sequence[int]) -> tuple[np.ndarray, bool]:
    """Message order sorted by block count, longest first (stable); (order, is_identity)."""
    ln = np.ascontiguousarray(length, dtype=np.uint32)
    order = np.empty(ln.size, dtype=np.uint32)
    rc = _lib.load().mirsha_bucket_order(_ptr(ln), ln.size, _ptr(order))
    if rc < 0:
        raise MirshaError(rc, "bucket_order")
    return order, bool(rc == 1)


def order_plan(n: int, min_len: int, max_len: int) -> tuple[int, int, int, int]:
    """Host-only mirsha_order_plan: (bins, chunk, n_chunks, scratch_bytes) of the
    device-built bucket order of n lengths within [min_len, max_len]; raises
    MirshaError (ERANGE) past MIRSHA_ORDER_MAX_BINS bins."""
    bins, chunk, n_chunks = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    scratch = ctypes.c_uint64(0)
    rc = _lib.load().mirsha_order_plan(int(n), int(min_len), int(max_len), ctypes.byref(bins), ctypes.byref(chunk),
                                       ctypes.byref(n_chunks), ctypes.byref(scratch))
    if rc != _lib.MIRSHA_OK:
        raise MirshaError(rc, f"order plan: {bins.value} bins")
    return bins.value, chunk.value, n_chunks.value, scratch.value


def hash_batch_multi(devices: Iterable[int], arena, off, length) -> np.ndarray:
    """Request-range sharding over several devices in one process; host gather."""
    devs = np.ascontiguousarray(list(devices), dtype=np.int32)
    a = _as_u8(arena)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    ln = np.ascontiguousarray(length, dtype=np.uint32)
    out = np.empty((o.size, 32), dtype=np.uint8)
    rc = _lib.load().mirsha_hash_batch_multi(_ptr(devs), devs.size, _ptr(a), a.size, _ptr(o), _ptr(ln), o.size, _ptr(out))
    check(rc)
    return out


class MultiEngine:
    """The multi-GPU drop-in (mirsha_multi, include/mirsha.h): one context
    per listed device, requests cut into contiguous ranges of equal bytes,
    each range packed, copied over its device's own PCIe link and hashed in
    parallel; digests in origin order.  A device may be listed twice (two
    contexts on one GPU: tests on a one-GPU box)."""

    def __init__(self, devices: Iterable[int]):
        self._lib = _lib.load()
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        h = ctypes.c_void_p()
        check(self._lib.mirsha_multi_create(_ptr(devs), int(devs.size), ctypes.byref(h)))
        self.handle = h
        self.devices = [int(d) for d in devs]
        self._outstanding = {}

    def _check(self, rc: int) -> None:
        if rc != _lib.MIRSHA_OK:
            raw = self._lib.mirsha_multi_last_error(self.handle)
            raise MirshaError(rc, raw.decode() if raw else "")

    def context(self, k: int):
        """The ctypes handle of device index k's context (owned by this object)."""
        return self._lib.mirsha_multi_ctx(self.handle, int(k))

    def set_variant(self, variant: int) -> None:
        for k in range(len(self.devices)):
            check(self._lib.mirsha_ctx_set_variant(self.context(k), int(variant)))

    def hash_slice_arrays(self, sl: "SliceArrays") -> np.ndarray:
        out = np.empty((sl.n, 32), dtype=np.uint8)
        if sl.n:
            self._check(self._lib.mirsha_hash_slices_multi(self.handle, sl.ptr_p, sl.len_p, sl.first_p, sl.n,
                                                           _ptr(out)))
        return out

    def hash_slices(self, requests) -> np.ndarray:
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        return self.hash_slice_arrays(sl)

    def hash_arena(self, arena, off, length, out=None) -> np.ndarray:
        """mirsha_hash_arena_multi: requests packed in one arena (offsets, lengths)."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        out = _out_rows(out, o.size)
        if o.size:
            self._check(self._lib.mirsha_hash_arena_multi(self.handle, _ptr(a), a.size, _ptr(o), _ptr(ln), o.size,
                                                          _ptr(out)))
        return out

    def host_empty(self, nbytes: int) -> np.ndarray:
        """Page-locked host memory usable by every device (mirsha_multi_host_alloc)."""
        p = ctypes.c_void_p()
        self._check(self._lib.mirsha_multi_host_alloc(self.handle, int(nbytes), ctypes.byref(p)))
        buf = (ctypes.c_uint8 * max(int(nbytes), 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=int(nbytes))
        import weakref

        weakref.finalize(buf, self._lib.mirsha_host_free, p.value)
        return arr

    def submit_slices(self, requests, dedup: bool = False) -> "Ticket":
        sl = requests if isinstance(requests, SliceArrays) else SliceArrays.from_requests(requests)
        out = np.empty((sl.n, 32), dtype=np.uint8)
        t = ctypes.c_uint64(0)
        self._check(self._lib.mirsha_submit_slices_multi(self.handle, sl.ptr_p, sl.len_p, sl.first_p, sl.n,
                                                         _ptr(out), _lib.MIRSHA_SUBMIT_DEDUP if dedup else 0,
                                                         ctypes.byref(t)))
        self._outstanding[t.value] = out
        for k in [k for k in self._outstanding if k <= t.value - ASYNC_SLOTS]:
            del self._outstanding[k]
        return Ticket(t.value, out)

    def submit_arena(self, arena, off, length, out=None) -> "Ticket":
        """mirsha_submit_arena_multi: Engine.submit_batch over every device."""
        a = _as_u8(arena)
        o = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        if o.shape != ln.shape:
            raise ValueError("off and len differ in length")
        n = int(o.size)
        out = _out_rows(out, n)
        t = ctypes.c_uint64(0)
        self._check(self._lib.mirsha_submit_arena_multi(self.handle, _ptr(a), a.size, _ptr(o), _ptr(ln), n, _ptr(out),
                                                        ctypes.byref(t)))
        self._outstanding[t.value] = (out, a)
        for k in [k for k in self._outstanding if k <= t.value - ASYNC_SLOTS]:
            del self._outstanding[k]
        return Ticket(t.value, out)

    def wait(self, ticket: "Ticket") -> np.ndarray:
        self._check(self._lib.mirsha_wait_multi(self.handle, ticket.value))
        for k in [k for k in self._outstanding if k <= ticket.value]:
            del self._outstanding[k]
        return ticket.out

    def poll(self, ticket: "Ticket") -> bool:
        done = ctypes.c_int(0)
        self._check(self._lib.mirsha_poll_multi(self.handle, ticket.value, ctypes.byref(done)))
        return bool(done.value)

    def last_cut(self) -> list:
        """First request of each device index in the last call, then n."""
        buf = (ctypes.c_uint32 * (len(self.devices) + 1))()
        n = self._lib.mirsha_multi_last_cut(self.handle, buf, len(buf))
        return list(buf)[:n]

    def host_profile(self, k: int) -> dict:
        buf = (ctypes.c_double * len(Engine.HOST_PHASES))()
        n = self._lib.mirsha_multi_host_profile(self.handle, int(k), buf, len(Engine.HOST_PHASES))
        if n < 0:
            self._check(n)
        return {key: buf[i] for i, key in enumerate(Engine.HOST_PHASES)}

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.mirsha_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = [
    "Engine",
    "MultiEngine",
    "CheckpointChains",
    "SliceArrays",
    "Ticket",
    "ExpectTicket",
    "CommitTicket",
    "dedup_plan",
    "dedup_rows",
    "expect_plan",
    "expect_bitmap",
    "commit_plan",
    "commit_seg_plan",
    "MIRSHA_COMMIT_CHECKPOINT",
    "Pipeline",
    "bucket_order",
    "device_count",
    "hash_batch_multi",
    "MIRSHA_NULL_INDEX",
    "KERNEL_MSGS",
    "KERNEL_LISTS",
    "KERNEL_GEN",
    "KERNEL_CHAIN",
    "KERNEL_FUSED",
    "KERNEL_OVERLAP",
    "KERNEL_VERIFY",
    "KERNEL_EXPECT",
    "KERNEL_ORDER",
    "order_plan",
    "mismatch_indices",
    "PIPELINE_SEQUENTIAL",
    "PIPELINE_FUSED",
    "PIPELINE_AUTO",
    "VARIANT_LDS",
    "VARIANT_DIRECT",
    "VARIANT_LOWOCC",
    "VARIANT_LDS_ONLY",
    "VARIANT_CU",
    "VARIANT_PAIR",
    "VARIANTS",
]
