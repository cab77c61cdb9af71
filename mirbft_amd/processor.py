"""Host-side mirror of the reference's Processor hash path (Python binding).

reference (Go, github.com/IBM/mirbft)              here
------------------------------------------------  -------------------------------------
type Hasher func() hash.Hash      processor.go:21  ``Hasher`` = callable returning ``GpuHash``
HashRequest{Data, Origin}   actions.go:157-164     ``HashRequest(data, origin)``
HashResult{Digest, Request} actions.go:224-230     ``HashResult(digest, request)``
ActionResults{Digests, Checkpoints} :218-221       ``ActionResults``
(*Processor).Process        processor.go:65-171    ``Processor.process`` (hash loop :129-143)
ProcessorWorkPool.Process   processor.go:447-470   ``ProcessorWorkPool.process``
Commit{Batch, Checkpoint}   actions.go:169-179     ``Commit(batch, checkpoint)``
CheckpointResult            actions.go:234-243     ``CheckpointResult(checkpoint, value)``
commit loop                 processor.go:145-168   ``Processor(log=DeviceLog(...))``

The commit loop: a cycle's ``actions.commits`` (batches and checkpoints, in
order) goes to the Processor's ``log`` in one call -- with a ``DeviceLog``
one kernel launch over the device-resident checkpoint chains
(``CheckpointChains.commit``) -- and ``ActionResults.checkpoints`` holds one
``CheckpointResult`` per checkpoint, in commit order.  Commits without a log
raise; a cycle without commits touches no log.
``async_commits=True``: ``submit()`` (and so ``ProcessorWorkPool.process``)
queues the cycle's commits as a ticket of the engine's ring
(``DeviceLog.submit_cycle`` -> ``CheckpointChains.submit_commit``, or
``StreamLog.submit_cycle`` -> ``HashStreams.submit``) ahead of the
hashing instead of applying them first, and ``PendingResults.wait()`` collects
them: commitInParallel beside hashInParallel (processor.go:447-470).

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
come back with the verdict); with ``dedup=True`` as well it is still one:
``Engine.submit_slices_expect_dedup`` hashes each distinct content once,
expectation or not, and its select kernel reads every request's digest from
its representative's row (a cycle without any expectation stays one
``submit_slices(dedup=True)``).  ``process()`` keeps its synchronous split
(``Engine.verify_slices`` for the requests with an expectation,
``hash_slices`` for the rest and, again, for the mismatches): above 32 MiB it
takes the pipelined staging route, which the ring does not have.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Any, Callable, Optional

import numpy as np

from ._lib import MIRSHA_COMMIT_CHECKPOINT, MIRSHA_NULL_INDEX
from .engine import STREAM_SUM_RESET, STREAM_WRITE, CheckpointChains, Engine, HashStreams, hasher_info


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
class Checkpoint:
    """mirbft.Checkpoint (actions.go:192-205); opaque to the log but for seq_no."""

    seq_no: int = 0
    network_config: Any = None
    clients_state: Any = None


@dataclass(eq=False)
class CommitBatch:
    """What the application log reads of a committed pb.QEntry: the digest of
    each request in order (recorder.go:222-223); ``None`` or ``b""`` is a null
    request, whose Write changes nothing."""

    digests: list = field(default_factory=list)
    seq_no: int = 0


@dataclass(eq=False)
class Commit:
    """mirbft.Commit (actions.go:169-179): a batch, or else a checkpoint."""

    batch: Optional[CommitBatch] = None
    checkpoint: Optional[Checkpoint] = None


@dataclass(eq=False)
class CheckpointResult:
    """mirbft.CheckpointResult (actions.go:234-243): ``checkpoint`` is the
    request of the Commit that asked for it, ``commit`` that Commit."""

    checkpoint: Checkpoint
    value: bytes
    commit: Optional[Commit] = None


@dataclass(eq=False)
class Actions:
    """Subset of mirbft.Actions (actions.go:18-52) the hash and commit paths read."""

    hash: list = field(default_factory=list)
    commits: list = field(default_factory=list)


@dataclass(eq=False)
class ActionResults:
    digests: list = field(default_factory=list)
    checkpoints: list = field(default_factory=list)


def _is_checkpoint(k: int, commit) -> bool:
    """Which of its two kinds commits[k] is."""
    if (commit.batch is None) == (commit.checkpoint is None):
        raise ValueError(f"commits[{k}]: exactly one of batch and checkpoint must be set")
    return commit.checkpoint is not None


def commit_programme(commits, n_nodes: int = 1):
    """Host-only: one cycle's ``actions.commits`` as the arguments of
    ``CheckpointChains.commit`` for nodes 0..n_nodes-1, which all commit the
    same entries (testengine: NodeState.Commit on every node,
    recorder.go:213-256).  Returns (table, op_chain, op_digest): the (m, 32)
    table holds each non-null request digest ONCE, in commit order, whatever
    the number of nodes; each step of the cycle is n_nodes consecutive ops
    (node 0 first), so value row ``j * n_nodes + node`` is checkpoint j's value
    on that node."""
    rows, prog = [], []
    for k, commit in enumerate(commits):
        if _is_checkpoint(k, commit):
            prog.append(MIRSHA_COMMIT_CHECKPOINT)
            continue
        for d in commit.batch.digests:
            if d is None or len(d) == 0:
                prog.append(MIRSHA_NULL_INDEX)
                continue
            if len(d) != 32:
                raise ValueError(f"commits[{k}]: a request digest of {len(d)} bytes")
            prog.append(len(rows))
            rows.append(bytes(d))
    table = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 32)
    op_digest = np.repeat(np.asarray(prog, dtype=np.uint32), n_nodes)
    op_chain = np.tile(np.arange(n_nodes, dtype=np.uint32), len(prog))
    return table, op_chain, op_digest


class _CycleLog:
    """What ``DeviceLog`` and ``StreamLog`` share: one cycle's
    ``actions.commits`` as ONE programme over a state object on the device (one
    state per node), run in one call or as a ticket of the engine's ring.  A
    subclass gives ``_cycle(commits)``, the arguments of its ``_run`` /
    ``_submit`` (the state object's synchronous and ring call)."""

    def __init__(self, engine: Engine, n_nodes: int, node: int, state, make):
        if not 0 <= node < n_nodes:
            raise ValueError(f"node {node} of {n_nodes}")
        self._engine = engine
        self.n_nodes, self.node = int(n_nodes), int(node)
        self._state = state if state is not None else make(engine, self.n_nodes)
        self.values = np.empty((0, self.n_nodes, 32), dtype=np.uint8)

    def _node_values(self, rows) -> list:
        self.values = rows.reshape(-1, self.n_nodes, 32)
        return [v.tobytes() for v in self.values[:, self.node]]

    def commit_cycle(self, commits) -> list:
        return self._node_values(self._run(*self._cycle(commits)))

    def submit_cycle(self, commits):
        """Queues one cycle's commits; returns the ticket ``collect_cycle`` takes."""
        return self._submit(*self._cycle(commits))

    def collect_cycle(self, ticket) -> list:
        """Waits for a cycle queued by ``submit_cycle``: node ``node``'s value
        per checkpoint, in commit order; ``values`` holds every node's."""
        return self._node_values(self._engine.wait(ticket))

    def close(self) -> None:
        self._state.close()


class DeviceLog(_CycleLog):
    """The application log of a Processor on the device: it stands where
    ``p.Log.Apply`` and ``p.Log.Snap`` stand in the commit loop
    (processor.go:147,163), with the testengine application's state
    (NodeState.ActiveHash, recorder.go:186-256) held in a ``CheckpointChains``.
    One cycle's ``actions.commits`` is ONE ``CheckpointChains.commit`` call.
    ``n_nodes = 1`` is a node's own log (chain 0); a testengine-style log
    drives the chains of n_nodes nodes, which commit the same entries, from the
    one cycle.  ``values`` keeps the last cycle's (checkpoints, n_nodes, 32)
    array; ``commit_cycle`` returns node ``node``'s.

    ``submit_cycle`` is the asynchronous form (``CheckpointChains.submit_commit``,
    a ticket of the engine's ring): the cycle is queued and the call returns;
    ``collect_cycle(ticket)`` waits for it and returns what ``commit_cycle``
    would have.  Cycles take effect in submission order, whatever the order
    they are collected in.

    The testengine log is made with the node's ``Hasher`` (recorder.go:186-256),
    so the chains hash with ``hasher`` ("sha256" or "sha512_256"; None: the
    engine's hasher as it is when the log is made).  Make the log after the
    engine's hasher is set (``Processor(engine, hasher=...)``): a log whose
    chains hash with another function than the engine raises MirshaError
    (MIRSHA_EINVAL) at the first commit."""

    def __init__(self, engine: Engine, n_nodes: int = 1, node: int = 0, chains=None, hasher=None):
        super().__init__(engine, n_nodes, node, chains, lambda eng, n: CheckpointChains(eng, n, hasher))
        self.chains = self._state
        self._run, self._submit = self.chains.commit, self.chains.submit_commit

    def _cycle(self, commits):
        return commit_programme(commits, self.n_nodes)


def batch_digests(batch) -> list:
    """``StreamLog``'s default ``entry_data``: the batch's non-null request
    digests, what the testengine log writes (recorder.go:222-223)."""
    out = []
    for d in batch.digests:
        if d is None or len(d) == 0:
            continue
        if len(d) != 32:
            raise ValueError(f"a request digest of {len(d)} bytes")
        out.append(bytes(d))
    return out


class StreamLog(_CycleLog):
    """``DeviceLog``'s interface over ``HashStreams``: an application log whose
    ``Apply`` writes ANY bytes (Log.Apply(*pb.QEntry) / Log.Snap are
    application-defined, processor.go:28-31), e.g. sequence numbers, payloads
    or a serialised entry.  ``entry_data(batch) -> list[bytes]`` is what Apply
    writes for a committed batch; the default writes its non-null request
    digests, which reproduces ``DeviceLog``'s checkpoint values.  A checkpoint
    is Sum-then-Reset.  One cycle's ``actions.commits`` is ONE
    ``HashStreams.run``: per commit n_nodes consecutive ops (node 0 first), so
    ``values`` is (checkpoints, n_nodes, 32) as ``DeviceLog``'s.  Every node's
    write op names the same range of the cycle's arena, and ``run`` sends each
    distinct range once: a cycle's bytes cross PCIe once, whatever n_nodes is.
    ``submit_cycle`` / ``collect_cycle`` are the asynchronous form
    (``HashStreams.submit``), with the contract of ``DeviceLog``'s: cycles take
    effect in submission order, whatever the order they are collected in.
    ``DeviceLog`` stays the log for digest-only applications.

    As ``DeviceLog``'s chains, the streams hash with ``hasher`` ("sha256" or
    "sha512_256"; None: the engine's hasher as it is when the log is made).
    Make the log after the engine's hasher is set (``Processor(engine,
    hasher=...)``): a log whose streams hash with another function than the
    engine raises MirshaError (MIRSHA_EINVAL) at the first commit."""

    def __init__(self, engine: Engine, n_nodes: int = 1, node: int = 0, entry_data=None, streams=None, hasher=None):
        super().__init__(engine, n_nodes, node, streams, lambda eng, n: HashStreams(eng, n, hasher))
        self.entry_data = entry_data if entry_data is not None else batch_digests
        self.streams = self._state
        self._run, self._submit = self.streams.run, self.streams.submit

    def cycle_programme(self, commits):
        """Host-only: (ops, arena) of one cycle for ``HashStreams.run``."""
        kinds, offs, lens, parts, at = [], [], [], [], 0
        for k, commit in enumerate(commits):
            if _is_checkpoint(k, commit):
                kinds.append(STREAM_SUM_RESET), offs.append(0), lens.append(0)
                continue
            data = b"".join(bytes(d) for d in self.entry_data(commit.batch))
            kinds.append(STREAM_WRITE), offs.append(at), lens.append(len(data))
            parts.append(data)
            at += len(data)
        n = self.n_nodes
        ops = (np.tile(np.arange(n, dtype=np.uint32), len(kinds)), np.repeat(np.asarray(kinds, dtype=np.uint32), n),
               np.repeat(np.asarray(offs, dtype=np.uint64), n), np.repeat(np.asarray(lens, dtype=np.uint32), n))
        return ops, b"".join(parts)

    _cycle = cycle_programme


class GpuHash:
    """hash.Hash (Write / Sum / Reset / Size / BlockSize) whose Sum runs on the
    GPU, with the engine's hasher: ``size`` / ``block_size`` are Go's Size() /
    BlockSize() of it, 32 / 64 for "sha256" and 32 / 128 for "sha512_256"."""

    def __init__(self, engine: Engine):
        self._engine = engine
        self._parts: list[bytes] = []

    @property
    def size(self) -> int:
        return hasher_info(self._engine.hasher)[0]

    @property
    def block_size(self) -> int:
        return hasher_info(self._engine.hasher)[1]

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

    def __init__(self, engine: Engine, reqs, ticket, parts=None, checkpoints=None, commit=None):
        """``ticket``: the cycle's one submission, or None; ``parts`` instead:
        [(ticket, request indices)] of a cycle split over several submissions.
        ``checkpoints``: the cycle's CheckpointResults (its commits were applied
        when it was submitted, so cycles commit in submission order).
        ``commit`` instead (``async_commits``): (log, ticket, the Commits that
        ask for a checkpoint) of a cycle whose commits were queued with
        ``log.submit_cycle``; ``wait()`` collects them."""
        self._engine, self._reqs, self._ticket = engine, reqs, ticket
        self._parts = parts
        self._checkpoints = checkpoints if checkpoints is not None else []
        self._commit = commit
        self._results: Optional[ActionResults] = None

    def _tickets(self):
        mine = [] if self._commit is None else [self._commit[1]]
        if self._parts is not None:
            return mine + [t for t, _ in self._parts]
        return mine if self._ticket is None else mine + [self._ticket]

    def _collect_commits(self) -> None:
        if self._commit is None:
            return
        log, ticket, asked = self._commit
        self._checkpoints = _checkpoint_results(asked, log.collect_cycle(ticket))
        self._commit = None

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
            self._collect_commits()  # queued first, retired first
            for ticket, idx in parts:
                self._part(ticket, idx, digests)
            # Digests[i] for actions.Hash[i] (processor.go:139)
            self._results = ActionResults(digests=[HashResult(digest=digests[i], request=r)
                                                   for i, r in enumerate(reqs)],
                                          checkpoints=self._checkpoints)
        return self._results


def _checkpoint_results(asked, values) -> list:
    """Checkpoints in commit order, each pointing back at its Commit
    (processor.go:164-167)."""
    if len(values) != len(asked):
        raise RuntimeError(f"the log returned {len(values)} values for {len(asked)} checkpoints")
    return [CheckpointResult(checkpoint=c.checkpoint, value=bytes(v), commit=c) for c, v in zip(asked, values)]


class Processor:
    """Hash stage of mirbft.Processor; batches one Ready() cycle per device call."""

    def __init__(self, engine: Optional[Engine] = None, device: int = 0, dedup: bool = False,
                 verify_on_device: bool = False, log=None, async_commits: bool = False, hasher=None):
        """``hasher``: the reference's ``Hasher`` (processor.go:21,58) by name,
        "sha256" or "sha512_256"; it is set on the engine (``Engine.set_hasher``)
        and so holds for every user of that engine.  None leaves the engine's
        hasher as it is (a new engine: "sha256").  A ``DeviceLog`` or a
        ``StreamLog`` takes the engine's hasher when it is made, so one made
        AFTER this Processor (and set as its ``log``) hashes its checkpoints
        with the same function, synchronously and with ``async_commits``; one
        made while the engine still hashed with another function raises
        MirshaError (MIRSHA_EINVAL) at the first commit.
        ``log``: the application log (p.Log, processor.go:147,163), e.g. a
        ``DeviceLog``: any object whose ``commit_cycle(commits)`` applies one
        cycle's commits and returns one value per checkpoint among them.
        ``async_commits``: ``submit()`` queues the cycle's commits
        (``log.submit_cycle``, if the log has it) instead of applying them
        before it queues the hashing, and ``PendingResults.wait()`` collects
        them (``log.collect_cycle``): commitInParallel beside hashInParallel
        (processor.go:447-470).  The ActionResults are the same either way."""
        self.engine = engine if engine is not None else Engine(device)
        if hasher is not None:
            self.engine.set_hasher(hasher)
        self.dedup = dedup
        self.verify_on_device = verify_on_device
        self.log = log
        self.async_commits = async_commits

    def process(self, actions: Actions) -> ActionResults:
        results = self._process_hash(actions.hash)  # the hash loop, then the commit loop
        results.checkpoints = self._commit(actions)
        return results

    def _commit(self, actions) -> list:
        """The commit loop (processor.go:145-168): the cycle's commits go to the
        log in one call; Checkpoints in commit order, each pointing back at
        its Commit.  No commits: nothing is called."""
        commits = list(getattr(actions, "commits", None) or [])
        if not commits:
            return []
        if self.log is None:  # the reference dereferences a nil p.Log
            raise RuntimeError("actions.commits without an application log (Processor(log=...))")
        asked = [c for c in commits if c.checkpoint is not None]
        return _checkpoint_results(asked, self.log.commit_cycle(commits))

    def _submit_commits(self, actions):
        """``async_commits``: the cycle's commits queued on the log, ahead of
        the hashing (so cycles commit in submission order whatever the order of
        the wait() calls).  Returns PendingResults' ``commit``, or None when
        there is nothing to collect."""
        commits = list(getattr(actions, "commits", None) or [])
        if not commits:
            return None
        if self.log is None:
            raise RuntimeError("actions.commits without an application log (Processor(log=...))")
        asked = [c for c in commits if c.checkpoint is not None]
        return (self.log, self.log.submit_cycle(commits), asked)

    def _process_hash(self, reqs) -> ActionResults:
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
        (``submit_slices_expect``); with ``dedup`` as well it is ONE
        deduplicated mixed submission (``submit_slices_expect_dedup``) when the
        cycle holds an expectation, else one ``submit_slices(dedup=True)``.
        An engine without ``submit_slices_expect_dedup`` gets the requests that
        carry an expectation in one ``submit_slices_expect`` and the rest in one
        ``submit_slices(dedup=True)``."""
        reqs = list(actions.hash)
        # The commits are applied here, synchronously and ahead of the hashing
        # (neither reads the other's results), so that cycles commit in
        # submission order whatever the order of the wait() calls.
        # With async_commits they are queued instead (the log's ring ticket,
        # ahead of the hashing tickets) and collected by wait().
        cps, cm = None, None
        if self.async_commits and hasattr(self.log, "submit_cycle"):
            cm = self._submit_commits(actions)
        else:
            cps = self._commit(actions)
        if not reqs:
            return PendingResults(self.engine, reqs, None, checkpoints=cps, commit=cm)
        if not self.verify_on_device:
            return PendingResults(self.engine, reqs, self.engine.submit_slices([r.data for r in reqs],
                                                                               dedup=self.dedup), checkpoints=cps,
                                  commit=cm)
        if not self.dedup:
            return PendingResults(self.engine, reqs, self.engine.submit_slices_expect(
                [r.data for r in reqs], [r.expected for r in reqs]), checkpoints=cps, commit=cm)
        check = [i for i, r in enumerate(reqs) if r.expected is not None]
        plain = [i for i, r in enumerate(reqs) if r.expected is None]
        if check and hasattr(self.engine, "submit_slices_expect_dedup"):
            return PendingResults(self.engine, reqs, self.engine.submit_slices_expect_dedup(
                [r.data for r in reqs], [r.expected for r in reqs]), checkpoints=cps, commit=cm)
        parts = []
        if check:
            parts.append((self.engine.submit_slices_expect([reqs[i].data for i in check],
                                                           [reqs[i].expected for i in check]), check))
        if plain:
            parts.append((self.engine.submit_slices([reqs[i].data for i in plain], dedup=True), plain))
        return PendingResults(self.engine, reqs, None, parts, checkpoints=cps, commit=cm)


class ProcessorWorkPool(Processor):
    """ProcessorWorkPool (processor.go:183-197): serialised Process, batched hashing.

    ``hash_workers`` is accepted for API parity (processor.go:396-399); the device
    replaces the goroutine pool.
    """

    def __init__(self, engine: Optional[Engine] = None, device: int = 0, hash_workers: int = 0,
                 transmit_workers: int = 0, dedup: bool = False, verify_on_device: bool = False, log=None,
                 async_commits: bool = False, hasher=None):
        super().__init__(engine, device, dedup, verify_on_device, log, async_commits, hasher)
        self._mutex = threading.Lock()
        self.hash_workers = hash_workers

    def process(self, actions: Actions, overlap: Optional[Callable[[], Any]] = None) -> ActionResults:
        """processor.go:447-470: the pool hashes while the WAL and the sends
        proceed.  Here the cycle's hashing is submitted first, ``overlap()``
        (the caller's persist / transmit work) runs while the GPU hashes, then
        the digests are collected in origin order -- with ``verify_on_device``
        too: the cycle's one mixed submission (``Processor.submit``) keeps the
        overlap.  With ``async_commits`` the cycle's commits are queued ahead of
        the hashing and collected with it: commits, hashing, ``overlap()``,
        wait -- the reference's shape."""
        with self._mutex:  # processor.go:448-449
            pending = self.submit(actions)
            if overlap is not None:
                overlap()
            return pending.wait()

    def stop(self) -> None:
        pass
