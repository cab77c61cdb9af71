"""The bucket order built on the device (mirsha_bucket_order_device: the count,
scan and scatter launches of mirsha_order.hip) against mirsha_bucket_order,
element for element; mirsha_offsets_device against numpy; and the chain
lengths -> offsets -> order -> digests with no host array in it."""
import numpy as np
import pytest

import oracle_py
import order_cases as oc
from mirbft_amd import MirshaError, _lib, bucket_order, order_plan

pytestmark = pytest.mark.gpu

FILL = 0xFFFFFFFF  # what an untouched order buffer holds


def _torch():
    import torch

    return torch


def device_order(engine, lens, min_len, max_len):
    """(order the device built, identity flag); the buffer starts as FILL."""
    torch = _torch()
    d_len = torch.from_numpy(lens.view(np.int32)).cuda()
    d_ord = torch.full((lens.size,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ident = engine.bucket_order_device(d_len.data_ptr(), lens.size, min_len, max_len, d_ord.data_ptr())
    engine.sync()
    return d_ord.cpu().numpy().view(np.uint32), ident


def check_equals_host(engine, lens, min_len, max_len):
    want, want_ident = bucket_order(lens)
    got, ident = device_order(engine, lens, min_len, max_len)
    assert np.array_equal(got, want)
    assert ident == want_ident == (order_plan(lens.size, min_len, max_len)[0] == 1)


@pytest.mark.parametrize("pattern", oc.PATTERNS)
def test_patterns_at_every_size(engine, pattern):
    for n in oc.SIZES:
        lens, lo, hi = oc.pattern_case(pattern, n)
        assert order_plan(n, lo, hi)[1] == oc.CHUNK  # the sizes sit around this plan's chunk
        check_equals_host(engine, lens, lo, hi)


def test_block_edges(engine):
    check_equals_host(engine, oc.EDGES, 0, 184)
    check_equals_host(engine, np.tile(oc.EDGES, 40)[::-1].copy(), 0, 184)


def test_loguniform_lengths(engine):
    lens, lo, hi = oc.loguniform()
    assert lens.size == 20_000 and order_plan(lens.size, lo, hi)[0] == 1024  # block counts 2 .. 1025
    check_equals_host(engine, lens, lo, hi)


def test_exactly_max_bins_and_one_more(engine):
    lens, lo, hi = oc.max_bins()
    assert order_plan(lens.size, lo, hi)[:3] == (_lib.MIRSHA_ORDER_MAX_BINS, 4096, 3)
    check_equals_host(engine, lens, lo, hi)
    # one bin more: refused, nothing queued, the output untouched
    longer = lens.copy()
    longer[longer.size // 3] = hi + 1
    with pytest.raises(MirshaError) as e:
        device_order(engine, longer, lo, hi + 1)
    assert e.value.code == _lib.MIRSHA_ERANGE
    torch = _torch()
    d_len = torch.from_numpy(longer.view(np.int32)).cuda()
    d_ord = torch.full((longer.size,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = engine._lib.mirsha_bucket_order_device(engine.ctx, d_len.data_ptr(), longer.size, lo, hi + 1,
                                                d_ord.data_ptr())
    engine.sync()
    assert rc == _lib.MIRSHA_ERANGE
    assert np.all(d_ord.cpu().numpy().view(np.uint32) == FILL)


def test_one_bin_is_the_identity(engine):
    for n in (1, 64, 65, 3000):
        lens = np.random.default_rng(n).integers(56, 120, n).astype(np.uint32)  # two blocks each
        got, ident = device_order(engine, lens, 56, 119)
        assert ident and np.array_equal(got, np.arange(n, dtype=np.uint32))
    # bounds of one block count decide it, whatever the lengths are
    got, ident = device_order(engine, np.array([5, 5000, 70], dtype=np.uint32), 60, 100)
    assert ident and got.tolist() == [0, 1, 2]


def test_lengths_outside_the_bounds_sort_as_the_nearest_bound(engine):
    rng = np.random.default_rng(3)
    for n in (65, 3000, 3 * oc.CHUNK + 17):
        lens = rng.integers(0, 5000, n).astype(np.uint32)
        lens[n // 2] = 0xFFFFFF00  # far past the bound
        got, ident = device_order(engine, lens, 500, 2000)
        assert not ident
        assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32))  # a permutation
        assert np.array_equal(got, oc.clamped_order(lens, 500, 2000))


def test_arguments(engine):
    torch = _torch()
    d = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib = engine._lib
    assert lib.mirsha_bucket_order_device(engine.ctx, d.data_ptr(), 8, 100, 99, d.data_ptr()) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_bucket_order_device(engine.ctx, None, 8, 0, 100, d.data_ptr()) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_bucket_order_device(engine.ctx, d.data_ptr(), 8, 0, 100, None) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_bucket_order_device(engine.ctx, None, 0, 0, 100, None) == 1  # n == 0: nothing to order
    assert lib.mirsha_offsets_device(engine.ctx, None, 8, d.data_ptr()) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_offsets_device(engine.ctx, d.data_ptr(), 8, None) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_offsets_device(engine.ctx, None, 0, None) == _lib.MIRSHA_OK
    engine.sync()


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_offsets_device(engine, n):
    torch = _torch()
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 1 << 31, n, dtype=np.int64).astype(np.uint32)
    want = np.zeros(n, dtype=np.uint64)
    np.cumsum(lens[:-1], dtype=np.uint64, out=want[1:])
    if n == 5000:
        assert int(want[-1]) > 1 << 32  # the sum leaves 32 bits
    d_len = torch.from_numpy(lens.view(np.int32)).cuda()
    d_off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    engine.offsets_device(d_len.data_ptr(), n, d_off.data_ptr())
    engine.sync()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want)


def test_device_only_chain(engine):
    """Config-5 lengths, their offsets, their order, their bytes and their
    digests, every array born on the device."""
    torch = _torch()
    seed, first, n = 0x6D69726266740005, 10**6 + 7, 4096
    min_len, max_len = 16 + 64, 16 + 65535  # the generator's range (oracle.h)
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_order = torch.empty(n, dtype=torch.int32, device="cuda")
    d_arena = torch.empty(n * max_len, dtype=torch.uint8, device="cuda")  # an upper bound: no length is read back
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    d_out_host_order = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.synth_mixed_lengths_device(seed, first, n, d_len.data_ptr())
    engine.offsets_device(d_len.data_ptr(), n, d_off.data_ptr())
    ident = engine.bucket_order_device(d_len.data_ptr(), n, min_len, max_len, d_order.data_ptr())
    engine.synth_mixed_device(seed, first, n, d_off.data_ptr(), d_arena.data_ptr())
    engine.hash_batch_device(d_arena.data_ptr(), d_arena.numel(), d_off.data_ptr(), d_len.data_ptr(),
                             d_order.data_ptr(), n, d_out.data_ptr())
    engine.sync()
    assert not ident
    lens = d_len.cpu().numpy().view(np.uint32)
    assert int(lens.min()) >= min_len and int(lens.max()) <= max_len
    host_order, _ = bucket_order(lens)
    assert np.array_equal(d_order.cpu().numpy().view(np.uint32), host_order)
    h_order = torch.from_numpy(host_order.view(np.int32)).cuda()
    torch.cuda.synchronize()
    engine.hash_batch_device(d_arena.data_ptr(), d_arena.numel(), d_off.data_ptr(), d_len.data_ptr(),
                             h_order.data_ptr(), n, d_out_host_order.data_ptr())
    engine.sync()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, d_out_host_order.cpu().numpy())
    pick = np.concatenate([np.arange(8), np.arange(n - 8, n), np.random.default_rng(9).choice(n, 64, replace=False)])
    arena_o, off_o, ln_o = oracle_py.gen_mixed(seed, (first + pick).astype(np.uint64))
    assert np.array_equal(ln_o, lens[pick])
    assert np.array_equal(got[pick], oracle_py.hash_requests(arena_o, off_o, ln_o))
