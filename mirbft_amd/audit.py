"""Audit of a recorded event log on the device.

Every HashResult an AddResults event records carries the digest the processor
produced and, in its Origin, what was hashed (``eventlog.origin_hash_data``
rebuilds the ``[][]byte`` for all five kinds).  ``audit_log`` gathers every
reconstructible result of a log, hashes them on the device and compares them
there with the recorded digests (``Engine.verify_slices``): only a verdict per
result comes back.  It works on any log written by ``eventlog.Recorder`` or by
the reference's ``eventlog`` package.

    python -m mirbft_amd.audit LOG

prints one JSON line with the report and exits 0 when every checked digest
matches, 1 when some do not, 2 when the log cannot be read.
"""
from __future__ import annotations

import dataclasses
import json
import sys
from typing import List, Optional, Sequence, Tuple

from . import eventlog


@dataclasses.dataclass
class AuditReport:
    checked: int = 0     # results compared (those with a malformed recorded digest included)
    skipped: int = 0     # results whose hashed bytes the log does not hold (redacted payloads)
    mismatches: List[Tuple[int, int]] = dataclasses.field(default_factory=list)  # (event index, result index)

    def to_json(self) -> str:
        return json.dumps({"checked": self.checked, "skipped": self.skipped, "n_mismatch": len(self.mismatches),
                           "mismatches": [list(m) for m in self.mismatches]})


def audit_log(events: Sequence[eventlog.RecordedEvent], engine, max_bytes: int = 1 << 30,
              hasher=None) -> AuditReport:
    """Re-hash and verify every reconstructible HashResult of ``events``.

    ``hasher``: the `Hasher` the recording node was configured with
    (processor.go:21,58), "sha256" or "sha512_256"; the engine hashes with it
    for this audit and has its own hasher back afterwards.  None: the engine's.

    ``engine.verify_slices(requests, expected)`` is called once per at most
    ``max_bytes`` of hash data (a single larger result gets a call of its own).
    A result whose recorded digest is not 32 bytes long is a mismatch without
    device work; a result whose payload was redacted counts as skipped."""
    if hasher is not None:
        before = engine.hasher
        engine.set_hasher(hasher)
        try:
            return audit_log(events, engine, max_bytes)
        finally:
            engine.set_hasher(before)
    report = AuditReport()
    where: List[Tuple[int, int]] = []
    data: List[List[bytes]] = []
    want: List[bytes] = []
    held = 0

    def flush() -> None:
        nonlocal held
        if where:
            for k in engine.verify_slices(data, want):
                report.mismatches.append(where[int(k)])
            where.clear()
            data.clear()
            want.clear()
        held = 0

    for ei, ev in enumerate(events):
        if not ev.state_event:
            continue
        for ri, hr in enumerate(eventlog.add_results_digests(ev.state_event)):
            _, digest, slices = eventlog.origin_hash_data(hr)
            if slices is None:
                report.skipped += 1
                continue
            report.checked += 1
            if len(digest) != 32:
                report.mismatches.append((ei, ri))
                continue
            size = sum(len(s) for s in slices)
            if where and held + size > max_bytes:
                flush()
            where.append((ei, ri))
            data.append(slices)
            want.append(digest)
            held += size
    flush()
    report.mismatches.sort()
    return report


def main(argv: Optional[Sequence[str]] = None, engine=None) -> int:
    args = list(sys.argv[1:] if argv is None else argv)
    hasher = None
    if "--hasher" in args:
        k = args.index("--hasher")
        if k + 1 < len(args):
            hasher = args[k + 1]
        del args[k:k + 2]
        from .engine import HASHERS

        if hasher not in HASHERS:
            print(f"--hasher: one of {sorted(HASHERS)}", file=sys.stderr)
            return 2
    if len(args) != 1:
        print("usage: python -m mirbft_amd.audit LOG [--hasher sha256|sha512_256]", file=sys.stderr)
        return 2
    try:
        with open(args[0], "rb") as f:
            events = list(eventlog.Reader(f))
    except (OSError, eventlog.EventLogError) as e:
        print(json.dumps({"error": str(e)}))
        return 2
    own = engine is None
    if own:
        from .engine import Engine

        engine = Engine(0)
    try:
        report = audit_log(events, engine, hasher=hasher)
    except eventlog.EventLogError as e:  # an event that does not parse
        print(json.dumps({"error": str(e)}))
        return 2
    finally:
        if own:
            engine.close()
    print(report.to_json())
    return 1 if report.mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
