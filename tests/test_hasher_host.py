"""Host-side surface of the pluggable hasher (no GPU): mirsha_hasher_info, the
NULL-context answers, the binding table, Engine.set_hasher's argument check,
and that the change which brought the second hasher left the SHA-256 kernel
sources (the inputs of bench.py's kernel_source_key) byte for byte alone."""
import ctypes
import gzip
import os
import subprocess

import pytest

from mirbft_amd import HASHERS, Engine, _lib, hasher_info
from mirbft_amd.processor import GpuHash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256_KERNEL_SOURCES = ["mirbft_amd/csrc/mirsha_kernels.hip", "mirbft_amd/csrc/mirsha_kernels.h",
                         "mirbft_amd/csrc/sha256_device.h", "mirbft_amd/csrc/sha256_rounds_asm.h"]


def test_hasher_info_values():
    lib = _lib.load()
    size, block = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert lib.mirsha_hasher_info(_lib.MIRSHA_HASHER_SHA256, ctypes.byref(size), ctypes.byref(block)) == _lib.MIRSHA_OK
    assert (size.value, block.value) == (32, 64)
    assert lib.mirsha_hasher_info(_lib.MIRSHA_HASHER_SHA512_256, ctypes.byref(size), ctypes.byref(block)) == _lib.MIRSHA_OK
    assert (size.value, block.value) == (32, 128)
    assert lib.mirsha_hasher_info(_lib.MIRSHA_HASHER_SHA512_256, None, None) == _lib.MIRSHA_OK
    for unknown in (2, -1, 256):
        size.value, block.value = 7, 9
        assert lib.mirsha_hasher_info(unknown, ctypes.byref(size), ctypes.byref(block)) == _lib.MIRSHA_EINVAL
        assert (size.value, block.value) == (7, 9)  # untouched
    assert hasher_info("sha256") == (32, 64) and hasher_info("sha512_256") == (32, 128)
    assert hasher_info(1) == (32, 128)


def test_null_context_is_einval():
    lib = _lib.load()
    assert lib.mirsha_ctx_set_hasher(None, _lib.MIRSHA_HASHER_SHA512_256) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_ctx_set_hasher(None, 99) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_ctx_hasher(None) == _lib.MIRSHA_EINVAL


def test_names_are_bound():
    for name in ("mirsha_ctx_set_hasher", "mirsha_ctx_hasher", "mirsha_hasher_info"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert HASHERS == {"sha256": 0, "sha512_256": 1}
    assert (_lib.MIRSHA_HASHER_SHA256, _lib.MIRSHA_HASHER_SHA512_256) == (0, 1)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


@pytest.mark.parametrize("bad", ["sha512", "SHA256", "", 2, -1])
def test_set_hasher_refuses_unknown_before_any_library_call(bad):
    eng = Engine.__new__(Engine)  # no context: the check must not need one
    eng._lib, eng.ctx = _NoLibrary(), None
    try:
        with pytest.raises(ValueError):
            eng.set_hasher(bad)
        with pytest.raises(ValueError):
            hasher_info(bad)
    finally:
        eng.ctx = None  # nothing for __del__ to close


def test_gpu_hash_sizes_follow_the_engines_hasher():
    class _Eng:
        hasher = "sha256"

    e = _Eng()
    g = GpuHash(e)
    assert (g.size, g.block_size) == (32, 64)
    e.hasher = "sha512_256"
    assert (g.size, g.block_size) == (32, 128)


def _git(*args):
    return subprocess.run(["git", *args], cwd=ROOT, capture_output=True, text=True)


def test_sha256_kernel_sources_untouched_by_the_hasher_change():
    """bench.py's traffic lookup keys on these four files: the change that
    added mirsha_sha512.hip must not differ from its parent in any of them
    (while that change is not committed yet, the parent is HEAD)."""
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    added = _git("log", "--diff-filter=A", "--format=%H", "--", "mirbft_amd/csrc/mirsha_sha512.hip").stdout.split()
    if added:
        parent = _git("rev-parse", "--verify", "--quiet", added[-1] + "~")
        if parent.returncode != 0:
            pytest.skip("the parent commit is not in this checkout (shallow clone)")
        r = _git("diff", "--quiet", parent.stdout.strip(), added[-1], "--", *SHA256_KERNEL_SOURCES)
    else:
        r = _git("diff", "--quiet", "HEAD", "--", *SHA256_KERNEL_SOURCES)
    assert r.returncode == 0, "a SHA-256 kernel source differs from the parent commit's"


class _FakeEngine:
    """Records what the audit does with the engine's hasher."""

    def __init__(self):
        self.hasher, self.calls = "sha256", []

    def set_hasher(self, h):
        self.calls.append(h)
        self.hasher = h

    def verify_slices(self, data, want):
        return []


def test_audit_hasher_option(tmp_path, capsys):
    from mirbft_amd import audit

    log = tmp_path / "empty.log"
    log.write_bytes(gzip.compress(b""))  # a log without events
    assert audit.main([str(log), "--hasher", "sha3"]) == 2  # refused before any engine exists
    assert audit.main(["--hasher"]) == 2
    assert "--hasher" in capsys.readouterr().err
    eng = _FakeEngine()
    assert audit.main([str(log), "--hasher", "sha512_256"], engine=eng) == 0
    assert eng.calls == ["sha512_256", "sha256"]  # set for the audit, the engine's own back afterwards
    eng = _FakeEngine()
    assert audit.main(["--hasher", "sha256", str(log)], engine=eng) == 0 and eng.calls == ["sha256", "sha256"]
    eng = _FakeEngine()
    assert audit.main([str(log)], engine=eng) == 0 and eng.calls == []  # no option: the engine's hasher
    assert audit.audit_log([], eng, hasher="sha512_256").checked == 0 and eng.hasher == "sha256"
