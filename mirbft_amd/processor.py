"""Host-side mirror of the reference's Processor hash path (Python binding).

reference (Go, github.com/IBM/mirbft)              here
------------------------------------------------  -------------------------------------
type Hasher func() hash.Hash      processor.go:21  ``Hasher`` = callable returning ``GpuHash``
HashRequest{Data, Origin}   actions.go:157-164     ``HashRequest(data, origin)``
HashResult{Digest, Request} actions.go:224-230     ``HashResult(digest, request)``
ActionResults{Digests, Checkpoints} :218-221       ``ActionResults``
(*Processor).Process        processor.go:65-171    ``Processor.process`` (hash loop :129-143)
ProcessorWorkPool.Process   processor.go:447-470   ``ProcessorWorkPool.process``

``Processor.process`` coalesces every HashRequest of one Ready() cycle into a
single batched device call and returns ``Digests[i]`` for ``actions.hash[i]``
with the request back-pointer (origin order).  The reference's work pool
returns digests in completion order (processor.go:349-356); this one keeps
origin order, which is a legal (and deterministic) completion order.
Failures raise (the reference panics, processor.go:75,81,85,91).

``dedup=True`` hashes each distinct request content once per cycle and hands
every duplicate its own digest (epoch-change acks: applyEpochChangeAckMsg,
epoch_target.go:459-477).  ``Processor.submit`` / ``PendingResults.wait`` is
the asynchronous form (mirsha_submit_slices / mirsha_wait): the cycle's
requests are packed before ``submit`` returns and the digests are collected,
in origin order, after the caller's other work for the cycle.

``verify_on_device=True``: a HashRequest that carries the digest its origin
expects (``expected``: RequestAck.Digest of a VerifyRequest,
state_machine.go:408-417; ExpectedDigest of a VerifyBatch,
batch_tracker.go:139-174) is hashed AND compared on the device, and only a
verdict comes back for it: a match yields ``digest = expected``, a mismatch
its true digest.  The results are the same ActionResults with the flag on or
off.  ``submit()`` (and so ``ProcessorWorkPool.process``) makes ONE ring
submission for the whole cycle, whatever it holds
(``Engine.submit_slices_expect``: the compare runs behind the hashing kernel,
and the digests of the requests without an expectation and of the mismatches
come back with the verdict); with ``dedup=True`` as well, the requests that
carry an expectation go in one such submission and the rest in one
``submit_slices(dedup=True)``.  ``process()`` keeps its synchronous split
(``Engine.verify_slices`` for the requests with an expectation,
``hash_slices`` for the rest and, again, for the mismatches): above 32 MiB it
takes the pipelined staging route, which the ring does not have.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Any, Callable, Optional

from .engine import Engine


@dataclass(eq=False)
class HashRequest:
    data: list  # [][]byte; concatenation is hashed
    origin: Any = None  # opaque to the hasher (actions.go:152-156)
    # The digest the origin expects (VerifyRequest / VerifyBatch), if it carries
    # one: read only by a Processor with verify_on_device=True.
    expected: Optional[bytes] = None


@dataclass(eq=False)
class HashResult:
    digest: bytes
    request: HashRequest


@dataclass(eq=False)
class Actions:
    """Subset of mirbft.Actions (actions.go:18-52) the hash path reads."""

    hash: list = field(default_factory=list)


@dataclass(eq=False)
class ActionResults:
    digests: list = field(default_factory=list)
    checkpoints: list = field(default_factory=list)


class GpuHash:
    """hash.Hash (Write / Sum / Reset / Size / BlockSize) whose Sum runs on the GPU."""

    size = 32
    block_size = 64

    def __init__(self, engine: Engine):
        self._engine = engine
        self._parts: list[bytes] = []

    def write(self, data: bytes) -> int:
        self._parts.append(bytes(data))
        return len(data)

    def sum(self, b: bytes = b"") -> bytes:
        return bytes(b) + self._engine.hash_slices([self._parts])[0].tobytes()

    def reset(self) -> None:
        self._parts = []


def gpu_hasher(engine: Engine) -> Callable[[], GpuHash]:
    """A `Hasher` factory (processor.go:21) backed by the GPU."""
    return lambda: GpuHash(engine)


def _results(reqs, digests) -> ActionResults:
    results = ActionResults(digests=[None] * len(reqs))
    for i, req in enumerate(reqs):  # Digests[i] for actions.Hash[i] (processor.go:139)
        results.digests[i] = HashResult(digest=digests[i].tobytes(), request=req)
    return results


class PendingResults:
    """Hash results of one submitted cycle; ``wait()`` returns its ActionResults."""

    def __init__(self, engine: Engine, reqs, ticket, parts=None):
        """``ticket``: the cycle's one submission, or None; ``parts`` instead:
        [(ticket, request indices)] of a cycle split over several submissions."""
        self._engine, self._reqs, self._ticket = engine, reqs, ticket
        self._parts = parts
        self._results: Optional[ActionResults] = None

    def _tickets(self):
        if self._parts is not None:
            return [t for t, _ in self._parts]
        return [] if self._ticket is None else [self._ticket]

    def done(self) -> bool:
        return self._results is not None or all(self._engine.poll(t) for t in self._tickets())

    def _part(self, ticket, idx, digests) -> None:
        """digests[idx[k]] = request k of one submission.  A mixed submission
        (``ticket.has``): a matching request's digest is its expectation (its
        row of ``out`` is not written), every other request's is its row."""
        out = self._engine.wait(ticket)
        has = getattr(ticket, "has", None)
        if has is None:
            for k, i in enumerate(idx):
                digests[i] = out[k].tobytes()
            return
        wrong = set(int(k) for k in ticket.mismatches)
        for k, i in enumerate(idx):
            match = bool(has[k]) and k not in wrong
            digests[i] = bytes(self._reqs[i].expected) if match else out[k].tobytes()

    def wait(self) -> ActionResults:
        if self._results is None:
            reqs = self._reqs
            parts = self._parts
            if parts is None:
                parts = [] if self._ticket is None else [(self._ticket, range(len(reqs)))]
            digests: list = [None] * len(reqs)
            for ticket, idx in parts:
                self._part(ticket, idx, digests)
            # Digests[i] for actions.Hash[i] (processor.go:139)
            self._results = ActionResults(digests=[HashResult(digest=digests[i], request=r)
                                                   for i, r in enumerate(reqs)])
        return self._results


class Processor:
    """Hash stage of mirbft.Processor; batches one Ready() cycle per device call."""

    def __init__(self, engine: Optional[Engine] = None, device: int = 0, dedup: bool = False,
                 verify_on_device: bool = False):
        self.engine = engine if engine is not None else Engine(device)
        self.dedup = dedup
        self.verify_on_device = verify_on_device

    def process(self, actions: Actions) -> ActionResults:
        reqs = actions.hash
        if not reqs:
            return ActionResults(digests=[])
        if self.verify_on_device:
            return self._process_verifying(reqs)
        return _results(reqs, self.engine.hash_slices([r.data for r in reqs], dedup=self.dedup))

    def _process_verifying(self, reqs) -> ActionResults:
        """One cycle split in two device calls: requests with ``expected`` are
        hashed and compared on the device, the rest hashed as usual.  Same
        ActionResults as the plain path (digests, order, back-pointers)."""
        check = [i for i, r in enumerate(reqs) if r.expected is not None]
        plain = [i for i, r in enumerate(reqs) if r.expected is None]
        digests: list = [None] * len(reqs)
        if check:
            bad = self.engine.verify_slices([reqs[i].data for i in check], [reqs[i].expected for i in check])
            wrong = [check[int(k)] for k in bad]
            for i in check:
                digests[i] = bytes(reqs[i].expected)
            plain = sorted(plain + wrong)  # mismatches: the true digest, with the rest of the cycle
        if plain:
            got = self.engine.hash_slices([reqs[i].data for i in plain], dedup=self.dedup)
            for k, i in enumerate(plain):
                digests[i] = got[k].tobytes()
        return ActionResults(digests=[HashResult(digest=digests[i], request=r) for i, r in enumerate(reqs)])

    def submit(self, actions: Actions) -> PendingResults:
        """Asynchronous process(): queue the cycle's hashing, return at once.
        With ``verify_on_device`` the whole cycle is ONE mixed submission
        (``submit_slices_expect``); with ``dedup`` as well, the requests that
        carry an expectation are one such submission and the rest one
        ``submit_slices(dedup=True)`` (the two do not combine in one)."""
        reqs = list(actions.hash)
        if not reqs:
            return PendingResults(self.engine, reqs, None)
        if not self.verify_on_device:
            return PendingResults(self.engine, reqs, self.engine.submit_slices([r.data for r in reqs],
                                                                               dedup=self.dedup))
        if not self.dedup:
            return PendingResults(self.engine, reqs, self.engine.submit_slices_expect(
                [r.data for r in reqs], [r.expected for r in reqs]))
        check = [i for i, r in enumerate(reqs) if r.expected is not None]
        plain = [i for i, r in enumerate(reqs) if r.expected is None]
        parts = []
        if check:
            parts.append((self.engine.submit_slices_expect([reqs[i].data for i in check],
                                                           [reqs[i].expected for i in check]), check))
        if plain:
            parts.append((self.engine.submit_slices([reqs[i].data for i in plain], dedup=True), plain))
        return PendingResults(self.engine, reqs, None, parts)


class ProcessorWorkPool(Processor):
    """ProcessorWorkPool (processor.go:183-197): serialised Process, batched hashing.

    ``hash_workers`` is accepted for API parity (processor.go:396-399); the device
    replaces the goroutine pool.
    """

    def __init__(self, engine: Optional[Engine] = None, device: int = 0, hash_workers: int = 0,
                 transmit_workers: int = 0, dedup: bool = False, verify_on_device: bool = False):
        super().__init__(engine, device, dedup, verify_on_device)
        self._mutex = threading.Lock()
        self.hash_workers = hash_workers

    def process(self, actions: Actions, overlap: Optional[Callable[[], Any]] = None) -> ActionResults:
        """processor.go:447-470: the pool hashes while the WAL and the sends
        proceed.  Here the cycle's hashing is submitted first, ``overlap()``
        (the caller's persist / transmit work) runs while the GPU hashes, then
        the digests are collected in origin order -- with ``verify_on_device``
        too: the cycle's one mixed submission (``Processor.submit``) keeps the
        overlap."""
        with self._mutex:  # processor.go:448-449
            pending = self.submit(actions)
            if overlap is not None:
                overlap()
            return pending.wait()

    def stop(self) -> None:
        pass
