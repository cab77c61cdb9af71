"""Host-side surface of the streams' hasher (no GPU): the three new entries
in the header, the library and the binding table; the sizes of an exported
state; the NULL answers; and the plain-Python SHA-512 compression of
tests/stream512ref.py, which the GPU tests' expected states come from, against
hashlib."""
import ctypes
import hashlib
import os
import re

from mirbft_amd import _lib, stream_state_bytes

import stream512ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (("mirsha_streams_create_hasher", 4), ("mirsha_streams_hasher", 1), ("mirsha_stream_state_bytes", 2))


def test_names_are_declared_exported_and_bound_with_the_headers_arity():
    with open(os.path.join(ROOT, "include", "mirsha.h")) as f:
        header = f.read()
    for name, arity in NEW:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define MIRSHA_STREAM_STATE_BYTES 108u\b", header)
    assert re.search(r"#define MIRSHA_STREAM_STATE_BYTES_SHA512 204u\b", header)


def test_stream_state_bytes():
    lib = _lib.load()
    n = ctypes.c_uint32(0)
    assert lib.mirsha_stream_state_bytes(_lib.MIRSHA_HASHER_SHA256, ctypes.byref(n)) == _lib.MIRSHA_OK and n.value == 108
    assert lib.mirsha_stream_state_bytes(_lib.MIRSHA_HASHER_SHA512_256, ctypes.byref(n)) == _lib.MIRSHA_OK
    assert n.value == 204 == _lib.MIRSHA_STREAM_STATE_BYTES_SHA512 == stream512ref.STATE_BYTES
    n.value = 5
    assert lib.mirsha_stream_state_bytes(7, ctypes.byref(n)) == _lib.MIRSHA_EINVAL and n.value == 5
    assert lib.mirsha_stream_state_bytes(_lib.MIRSHA_HASHER_SHA512_256, None) == _lib.MIRSHA_OK
    assert (stream_state_bytes("sha256"), stream_state_bytes("sha512_256")) == (108, 204)


def test_null_arguments_are_einval():
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.mirsha_streams_create_hasher(None, 1, _lib.MIRSHA_HASHER_SHA512_256, ctypes.byref(out)) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_streams_hasher(None) == _lib.MIRSHA_EINVAL


def test_the_plain_python_compression_is_sha512_256():
    for msg in (b"abc", bytes(300), b"", bytes(range(256)) * 3):
        assert stream512ref.sha512_256_by_hand(msg) == hashlib.new("sha512_256", msg).digest()
    assert stream512ref.sha512_256_by_hand(b"").hex() == \
        "c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a"
    # a state is its midstate, the buffered tail and the length: continuing from it is continuing the message
    data = bytes(range(251)) * 2
    st = stream512ref.marshal_of(data[:300])
    assert len(st) == 204 and st[:4] == b"sha\x06" and st[-8:] == (300).to_bytes(8, "big")
    h = [int.from_bytes(st[4 + 8 * i:12 + 8 * i], "big") for i in range(8)]
    assert stream512ref.continue_from(h, st[68:68 + 300 % 128], 300, data[300:]) == \
        hashlib.new("sha512_256", data).digest()
