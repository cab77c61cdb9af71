"""Encoders of the HashResult messages an event log records
(mirbftpb/mirbft.proto:408-448), for the verify / audit tests: each returns
the encoded HashResult with the digest hashlib gives for its origin, or
`digest` in its place (a tampered record)."""
import hashlib

from mirbft_amd import eventlog as el, hashdata


def request_msg(cid, rno, data):
    return el.f_uint(1, cid) + el.f_uint(2, rno) + el.f_bytes(3, data)


def ack_msg(cid, rno, digest):
    return el.f_uint(1, cid) + el.f_uint(2, rno) + el.f_bytes(3, digest)


def sha(slices):
    return hashlib.sha256(b"".join(slices)).digest()


def request_result(src, cid, rno, data, digest=None):
    d = sha(hashdata.request_hash_data(cid, rno, data)) if digest is None else digest
    return el.f_bytes(1, d) + el.f_msg(el.HR_REQUEST, el.f_uint(1, src) + el.f_msg(2, request_msg(cid, rno, data)))


def verify_request_result(src, cid, rno, data, digest=None):
    d = sha(hashdata.request_hash_data(cid, rno, data))
    body = el.f_uint(1, src) + el.f_msg(2, ack_msg(cid, rno, d)) + el.f_bytes(3, data)
    return el.f_bytes(1, d if digest is None else digest) + el.f_msg(el.HR_VERIFY_REQUEST, body)


def batch_result(src, epoch, seq, ack_digests, digest=None):
    # an ack message is present even when its digest is empty (a null request)
    acks = b"".join(el.f_msg(5, ack_msg(1, i, d)) for i, d in enumerate(ack_digests))
    body = el.f_uint(1, src) + el.f_uint(2, epoch) + el.f_uint(3, seq) + acks
    return el.f_bytes(1, sha(ack_digests) if digest is None else digest) + el.f_msg(el.HR_BATCH, body)


def verify_batch_result(src, seq, ack_digests, digest=None):
    d = sha(ack_digests)
    acks = b"".join(el.f_msg(3, ack_msg(2, i, a)) for i, a in enumerate(ack_digests))
    body = el.f_uint(1, src) + el.f_uint(2, seq) + acks + el.f_bytes(4, d)
    return el.f_bytes(1, d if digest is None else digest) + el.f_msg(el.HR_VERIFY_BATCH, body)


def epoch_change_msg(new_epoch, cps, p_set, q_set):
    out = el.f_uint(1, new_epoch)
    out += b"".join(el.f_msg(2, el.f_uint(1, s) + el.f_bytes(2, v)) for s, v in cps)
    for num, entries in ((3, p_set), (4, q_set)):
        out += b"".join(el.f_msg(num, el.f_uint(1, e) + el.f_uint(2, s) + el.f_bytes(3, d)) for e, s, d in entries)
    return out


def epoch_change_result(src, origin, new_epoch, cps, p_set, q_set, digest=None):
    d = sha(hashdata.epoch_change_hash_data(new_epoch, cps, p_set, q_set))
    body = el.f_uint(1, src) + el.f_uint(2, origin) + el.f_msg(3, epoch_change_msg(new_epoch, cps, p_set, q_set))
    return el.f_bytes(1, d if digest is None else digest) + el.f_msg(el.HR_EPOCH_CHANGE, body)


def add_results(results):
    return el.f_msg(el.SE_ADD_RESULTS, b"".join(el.f_msg(1, r) for r in results))
