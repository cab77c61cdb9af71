"""The device-built bucket order, host side (no GPU): mirsha_order_plan against
a Python restatement of its rule, and a numpy restatement of the three launches
(per-chunk histograms, a bin-major exclusive scan, a stable scatter), with
`chunk` and `bins` taken from the plan, against mirsha_bucket_order -- the
algebra the kernels of mirsha_order.hip implement, pinned before a GPU runs it."""
import ctypes

import numpy as np
import pytest

import order_cases as oc
from mirbft_amd import MirshaError, _lib, bucket_order, order_plan


def plan_restated(n, min_len, max_len):
    bins = int(oc.blocks(max_len)) - int(oc.blocks(min_len)) + 1
    chunk = max(1024, (bins + 63) // 64 * 64)
    n_chunks = (n + chunk - 1) // chunk
    return bins, chunk, n_chunks, 8 * bins * n_chunks


@pytest.mark.parametrize("n", [0, 1, 63, 1023, 1024, 1025, 20_000, 1 << 20, 0xFFFFFFFF])
@pytest.mark.parametrize("min_len,max_len", [(0, 0), (0, 55), (0, 56), (80, 616), (64, 65536), (55, 56),
                                             (0, int(oc.longest_of(oc.MAX_BINS))), (1000, 1000 + 64 * 4095),
                                             (0xFFFFFF00 - 64 * 4095, 0xFFFFFF00)])
def test_plan_matches_its_rule(n, min_len, max_len):
    bins, chunk, n_chunks, scratch = order_plan(n, min_len, max_len)
    assert (bins, chunk, n_chunks, scratch) == plan_restated(n, min_len, max_len)
    assert 1 <= bins <= _lib.MIRSHA_ORDER_MAX_BINS
    assert chunk % 64 == 0 and chunk >= bins
    assert n_chunks == (n + chunk - 1) // chunk
    assert scratch <= 8 * n + 65536
    if n == 0:
        assert n_chunks == 0 and scratch == 0


def test_plan_bin_cap():
    top = int(oc.longest_of(oc.MAX_BINS))  # 4096 blocks
    assert order_plan(5000, 0, top)[0] == 4096 == _lib.MIRSHA_ORDER_MAX_BINS
    with pytest.raises(MirshaError) as e:
        order_plan(5000, 0, top + 1)  # 4097 blocks
    assert e.value.code == _lib.MIRSHA_ERANGE
    # the raw call reports the bin count and zeroes the rest
    out = [ctypes.c_uint32(9) for _ in range(3)]
    scratch = ctypes.c_uint64(9)
    rc = _lib.load().mirsha_order_plan(5000, 0, top + 1, *[ctypes.byref(v) for v in out], ctypes.byref(scratch))
    assert rc == _lib.MIRSHA_ERANGE and [v.value for v in out] == [4097, 0, 0] and scratch.value == 0


def test_plan_bad_arguments():
    lib = _lib.load()
    v = ctypes.c_uint32(0)
    s = ctypes.c_uint64(0)
    assert lib.mirsha_order_plan(10, 5, 4, v, v, v, s) == _lib.MIRSHA_EINVAL
    for k in range(3):
        args = [v, v, v]
        args[k] = None
        assert lib.mirsha_order_plan(10, 0, 100, *args, s) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_order_plan(10, 0, 100, v, v, v, None) == _lib.MIRSHA_EINVAL


def check_three_passes(lens, min_len, max_len):
    bins, chunk, n_chunks, _ = order_plan(lens.size, min_len, max_len)
    want, ident = bucket_order(lens)
    got = oc.three_passes(lens, min_len, max_len, bins, chunk, n_chunks)
    assert np.array_equal(got, want)
    assert ident == (bins == 1) or lens.size == 0
    return bins, chunk, n_chunks


@pytest.mark.parametrize("pattern", oc.PATTERNS)
@pytest.mark.parametrize("n", oc.SIZES)
def test_three_passes_reproduce_the_host_order(pattern, n):
    lens, lo, hi = oc.pattern_case(pattern, n)
    _, chunk, n_chunks = check_three_passes(lens, lo, hi)
    assert chunk == oc.CHUNK  # the sizes are chunk - 1, chunk, chunk + 1, 3 chunk + 17 of this plan
    assert n_chunks == (n + chunk - 1) // chunk


def test_three_passes_block_edges():
    lens = np.tile(oc.EDGES, 40)[::-1].copy()
    bins, _, _ = check_three_passes(lens, 0, 184)
    assert bins == 4


def test_three_passes_loguniform_and_max_bins():
    lens, lo, hi = oc.loguniform()
    bins, chunk, n_chunks = check_three_passes(lens, lo, hi)
    assert bins == 1024 and n_chunks > 1  # blocks 2 .. 1025
    lens, lo, hi = oc.max_bins()
    bins, chunk, n_chunks = check_three_passes(lens, lo, hi)
    assert (bins, chunk, n_chunks) == (4096, 4096, 3)


def test_three_passes_clamp_lengths_outside_the_bounds():
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 5000, 3000).astype(np.uint32)
    bins, chunk, n_chunks, _ = order_plan(lens.size, 500, 2000)
    got = oc.three_passes(lens, 500, 2000, bins, chunk, n_chunks)
    assert np.array_equal(got, oc.clamped_order(lens, 500, 2000))
    assert np.array_equal(np.sort(got), np.arange(lens.size))


def test_binding_has_the_new_entry_points():
    lib = _lib.load()
    for name in ("mirsha_order_plan", "mirsha_bucket_order_device", "mirsha_offsets_device",
                 "mirsha_ctx_set_order_mode", "mirsha_ctx_order_mode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # NULL contexts are refused before anything touches a device
    assert lib.mirsha_ctx_set_order_mode(None, 1) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_ctx_order_mode(None) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_bucket_order_device(None, None, 0, 0, 0, None) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_offsets_device(None, None, 0, None) == _lib.MIRSHA_EINVAL
