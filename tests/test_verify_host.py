"""Host side of digest verification (no GPU): eventlog.origin_hash_data for the
five HashResult kinds against hashlib over the golden layouts
(tests/golden/layouts.json), audit_log with a hashlib stand-in engine, the
bitmap -> index helper and the HashRequest constructor."""
import hashlib
import io

import numpy as np
import pytest

from mirbft_amd import HashRequest, eventlog as el, hashdata, mismatch_indices
from mirbft_amd.audit import AuditReport, audit_log, main as audit_main

from hashresult_pb import (add_results, batch_result, epoch_change_result, request_result, sha, verify_batch_result,
                           verify_request_result)


# ---- origin_hash_data against the golden layouts -----------------------------

def test_origin_request_and_verify_request(layouts):
    for e in layouts["testengine_requests"][::37]:
        c, r = e["client"], e["req_no"]
        payload = hashdata.testengine_request_payload(c, r)
        for make, kind in ((request_result, el.HR_REQUEST), (verify_request_result, el.HR_VERIFY_REQUEST)):
            k, digest, data = el.origin_hash_data(make(3, c, r, payload))
            assert k == kind and digest.hex() == e["sha256"]
            assert data == hashdata.request_hash_data(c, r, payload)  # client 0 / reqNo 0: absent fields read as 0
            assert sha(data).hex() == e["sha256"]


def test_origin_redacted_request_has_no_data():
    ev = add_results([request_result(1, 5, 6, b"abc"), verify_request_result(2, 5, 7, b"xyz")])
    for hr in el.add_results_digests(el.redact_event(ev)):
        kind, digest, data = el.origin_hash_data(hr)
        assert kind in (el.HR_REQUEST, el.HR_VERIFY_REQUEST) and len(digest) == 32 and data is None


def test_origin_batch_and_verify_batch_with_nulls(layouts):
    req = {(e["client"], e["req_no"]): bytes.fromhex(e["sha256"]) for e in layouts["testengine_requests"]}
    assert any(k is None for b in layouts["batches"] for k in b["entries"])
    for b in layouts["batches"]:
        acks = [b"" if k is None else req[tuple(k)] for k in b["entries"]]
        for hr, kind in ((batch_result(1, 2, 9, acks), el.HR_BATCH), (verify_batch_result(1, 9, acks), el.HR_VERIFY_BATCH)):
            k, digest, data = el.origin_hash_data(hr)
            assert k == kind and digest.hex() == b["sha256"], b["name"]
            assert data == acks, b["name"]  # one slice per ack, empty digests kept
            assert sha(data).hex() == b["sha256"]


def test_origin_epoch_change(layouts):
    ec = layouts["epoch_change"]
    cps = [(s, bytes.fromhex(v)) for s, v in ec["checkpoints"]]
    p_set = [(e, s, bytes.fromhex(d)) for e, s, d in ec["p_set"]]
    q_set = [(e, s, bytes.fromhex(d)) for e, s, d in ec["q_set"]]
    kind, digest, data = el.origin_hash_data(epoch_change_result(2, 1, ec["new_epoch"], cps, p_set, q_set))
    assert kind == el.HR_EPOCH_CHANGE and digest.hex() == ec["sha256"]
    assert len(data) == ec["n_slices"] and sha(data).hex() == ec["sha256"]
    # checkpoint seq_no 0 is absent on the wire and reads back as 0
    assert cps[0][0] == 0 and data[1] == bytes(8)
    # an EpochChange with nothing set: just LE64(0)
    kind, _, data = el.origin_hash_data(epoch_change_result(0, 0, 0, [], [], []))
    assert kind == el.HR_EPOCH_CHANGE and data == [bytes(8)]


def test_origin_without_a_kind():
    assert el.origin_hash_data(el.f_bytes(1, b"d" * 32)) == (0, b"d" * 32, None)
    assert el.add_results_digests(el.tick_event()) == []


# ---- audit_log ----------------------------------------------------------------

class HashlibEngine:
    """CPU stand-in with Engine.verify_slices' signature; records its calls."""

    def __init__(self):
        self.calls = []

    def verify_slices(self, requests, expected):
        self.calls.append(sum(len(s) for r in requests for s in r))
        assert all(len(e) == 32 for e in expected)
        return np.asarray([i for i, (r, e) in enumerate(zip(requests, expected)) if sha(r) != e], dtype=np.int64)


def five_kinds(i, tamper=None):
    """One AddResults event with one result of each kind; `tamper` = position whose recorded digest is altered."""
    d = [hashlib.sha256(b"%d-%d" % (i, k)).digest() for k in range(8)]
    wrong = lambda pos: bytes(32) if tamper == pos else None  # noqa: E731
    return add_results([
        request_result(1, i, 2 * i, b"payload-%d" % i, wrong(0)),
        verify_request_result(2, i, 2 * i + 1, b"fwd-%d" % i, wrong(1)),
        batch_result(0, 1, i, [d[0], b"", d[1]], wrong(2)),
        verify_batch_result(3, i, d[2:5], wrong(3)),
        epoch_change_result(1, 2, 7, [(20, d[5])], [(6, 21, d[6])], [(6, 21, d[7])], wrong(4)),
    ])


def logged(events, retain=True):
    out = io.BytesIO()
    rec = el.Recorder(1, out, time_source=lambda: 0, retain_request_data=retain)
    for ev in events:
        rec.intercept(ev)
    rec.stop()
    return out.getvalue()


def read(raw):
    return list(el.Reader(io.BytesIO(raw)))


def test_audit_clean_log():
    events = [el.tick_event() if i % 3 == 0 else five_kinds(i) for i in range(30)]
    eng = HashlibEngine()
    rep = audit_log(read(logged(events)), eng)
    assert rep == AuditReport(checked=100, skipped=0, mismatches=[])
    assert len(eng.calls) == 1


@pytest.mark.parametrize("pos", range(5))
def test_audit_tampered_digest_of_each_kind(pos):
    events = [el.tick_event(), five_kinds(1), five_kinds(2, tamper=pos), five_kinds(3)]
    rep = audit_log(read(logged(events)), HashlibEngine())
    assert rep.checked == 15 and rep.skipped == 0 and rep.mismatches == [(2, pos)]


def test_audit_short_recorded_digest_needs_no_device_work():
    bad = batch_result(0, 1, 4, [b"a" * 32], digest=b"x" * 31)
    eng = HashlibEngine()
    rep = audit_log(read(logged([add_results([bad])])), eng)
    assert rep == AuditReport(checked=1, skipped=0, mismatches=[(0, 0)]) and eng.calls == []
    rep = audit_log(read(logged([five_kinds(1), add_results([request_result(1, 2, 3, b"p"), bad])])), eng)
    assert rep.checked == 7 and rep.mismatches == [(1, 1)] and len(eng.calls) == 1


def test_audit_redacted_log_skips_requests_checks_batches():
    events = [five_kinds(i) for i in range(6)]
    rep = audit_log(read(logged(events, retain=False)), HashlibEngine())
    # Request and VerifyRequest of every event are redacted; the other three kinds are still checked
    assert rep == AuditReport(checked=18, skipped=12, mismatches=[])
    events[4] = five_kinds(4, tamper=2)
    rep = audit_log(read(logged(events, retain=False)), HashlibEngine())
    assert rep.skipped == 12 and rep.mismatches == [(4, 2)]


def test_audit_chunks_by_max_bytes():
    results = [request_result(1, i, i, bytes(84)) for i in range(12)]  # 100 bytes of hash data each
    results[7] = request_result(1, 7, 7, bytes(84), digest=bytes(32))
    events = read(logged([add_results(results[:5]), add_results(results[5:])]))
    eng = HashlibEngine()
    rep = audit_log(events, eng, max_bytes=400)
    assert eng.calls == [400, 400, 400]
    assert rep.checked == 12 and rep.mismatches == [(1, 2)]
    one = HashlibEngine()
    assert audit_log(events, one).mismatches == [(1, 2)] and one.calls == [1200]
    # a single result above the limit still gets its own call
    tiny = HashlibEngine()
    assert audit_log(events, tiny, max_bytes=10).mismatches == [(1, 2)] and tiny.calls == [100] * 12


def test_audit_cli_exit_codes(tmp_path, capsys):
    import json

    good, bad, junk = tmp_path / "good.gz", tmp_path / "bad.gz", tmp_path / "junk.gz"
    good.write_bytes(logged([five_kinds(1), five_kinds(2)]))
    bad.write_bytes(logged([five_kinds(1), five_kinds(2, tamper=3)]))
    junk.write_bytes(b"not a gzip stream at all")
    assert audit_main([str(good)], engine=HashlibEngine()) == 0
    assert json.loads(capsys.readouterr().out) == {"checked": 10, "skipped": 0, "n_mismatch": 0, "mismatches": []}
    assert audit_main([str(bad)], engine=HashlibEngine()) == 1
    assert json.loads(capsys.readouterr().out)["mismatches"] == [[1, 3]]
    assert audit_main([str(junk)], engine=HashlibEngine()) == 2
    assert audit_main([str(tmp_path / "missing.gz")], engine=HashlibEngine()) == 2
    assert audit_main([str(good)[:-3]], engine=HashlibEngine()) == 2


# ---- small public pieces ------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_mismatch_indices(n):
    rng = np.random.default_rng(n)
    flags = rng.random(n) < 0.3
    if n:
        flags[-1] = True
    words = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)  # one spare word: ignored
    for i in np.flatnonzero(flags):
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    got = mismatch_indices(words, n)
    assert got.tolist() == np.flatnonzero(flags).tolist()
    if n % 64:  # bits of the last word at or beyond n are not items
        words[(n - 1) >> 6] |= np.uint64(1) << np.uint64(n % 64)
        assert mismatch_indices(words, n).tolist() == got.tolist()
    if n:
        with pytest.raises(ValueError):
            mismatch_indices(words[:(n + 63) // 64 - 1], n)


def test_expected_digests_array_and_sequence_forms():
    from mirbft_amd.engine import _expected_rows

    rows = np.arange(96, dtype=np.uint8).reshape(3, 32)
    arr, short = _expected_rows(rows, 3)
    assert np.array_equal(arr, rows) and short.size == 0
    seq = [rows[0].tobytes(), rows[1].tobytes()[:31], bytearray(rows[2].tobytes()), b""]
    arr, short = _expected_rows(seq, 4)
    # entries of another length: flagged on the host, 32 zero bytes for the device
    assert short.tolist() == [1, 3] and arr.shape == (4, 32)
    assert np.array_equal(arr[[0, 2]], rows[[0, 2]]) and not arr[[1, 3]].any()
    for bad in (rows[:2], rows.astype(np.uint16)):
        with pytest.raises(ValueError):
            _expected_rows(bad, 3)
    with pytest.raises(ValueError):
        _expected_rows(seq[:3], 4)


def test_hash_request_still_constructs_positionally():
    r = HashRequest([b"a", b"b"], "origin")
    assert r.data == [b"a", b"b"] and r.origin == "origin" and r.expected is None
    assert HashRequest([b"x"]).origin is None
    assert HashRequest([b"x"], None, b"d" * 32).expected == b"d" * 32
