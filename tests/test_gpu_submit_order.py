"""mirsha_submit_batch / mirsha_submit_batch_expect with the bucket order built
on the device (Engine.set_order_mode("device")) against the host mode on one
engine: the digests are byte-identical to each other and to the oracle, on
every arena route, and only a cycle of several block counts inside the bin cap
launches the order kernels (timing id 8)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_py
from mirbft_amd import MirshaError, _lib
from mirbft_amd.engine import KERNEL_ORDER

pytestmark = pytest.mark.gpu

ROUTES = {"gapless": 0, "gaps": 5, "sparse": 2000}  # bytes between messages; sparse: span > 2 x bytes + 4096
SIZES = (1, 65, 1000, 5000)


@functools.lru_cache(maxsize=None)
def cycle(n, gap, seed=0):
    """Mixed 0-600 B lengths (block counts 1..10), `gap` bytes apart; (src, off, len, oracle digests)."""
    rng = np.random.default_rng(1000 * n + gap + seed)
    lens = rng.integers(0, 601, n).astype(np.uint32)
    if n > 8:
        lens[::9] = 0
        lens[1:8] = [55, 56, 119, 120, 183, 184, 600]
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(gap))
    src = rng.integers(0, 256, int(off[-1]) + int(lens[-1]) + 1, dtype=np.uint8)
    want = oracle_py.hash_requests(src, off, lens)
    for a in (src, off, lens, want):
        a.setflags(write=False)
    return src, off, lens, want


@pytest.fixture
def eng(engine):
    """The session's engine; the mode and the timing are put back afterwards."""
    assert engine.order_mode == "host"  # the default
    yield engine
    engine.set_order_mode("host")
    engine.set_timing(False)


def order_launches(engine):
    return engine.kernel_time(KERNEL_ORDER)[0]


@pytest.mark.parametrize("pinned_out", [True, False])
@pytest.mark.parametrize("pinned_arena", [True, False])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_device_mode_equals_host_mode_and_the_oracle(eng, route, pinned_arena, pinned_out):
    for n in SIZES:
        src, off, lens, want = cycle(n, ROUTES[route])
        if route == "sparse" and n > 1:
            assert int(off[-1]) + int(lens[-1]) - int(off[0]) > 2 * int(lens.sum()) + 4096
        arena = eng.host_empty(src.size) if pinned_arena else np.empty(src.size, dtype=np.uint8)
        arena[:] = src
        got = {}
        for mode in ("host", "device"):
            eng.set_order_mode(mode)
            assert eng.order_mode == mode
            out = eng.host_empty(32 * n).reshape(n, 32) if pinned_out else np.empty((n, 32), dtype=np.uint8)
            out[:] = 0xA5
            got[mode] = eng.wait(eng.submit_batch(arena, off, lens, out=out)).copy()
        assert np.array_equal(got["device"], got["host"]), n
        assert np.array_equal(got["device"], want), n


def test_only_a_mixed_cycle_launches_the_order_kernels(eng):
    eng.set_order_mode("device")
    eng.set_timing(True)
    eng.reset_timing()
    n = 3000
    src = oracle_py.gen_requests(7, 0, n, 256)
    off = np.arange(n, dtype=np.uint64) * 272
    lens = np.full(n, 272, dtype=np.uint32)
    got = eng.wait(eng.submit_batch(src, off, lens))
    assert np.array_equal(got, oracle_py.hash_requests(src, off, lens))
    assert order_launches(eng) == 0  # one block count: the identity, no order launch
    src, off, lens, want = cycle(5000, 0)
    assert np.array_equal(eng.wait(eng.submit_batch(src, off, lens)), want)
    assert order_launches(eng) == 2  # count and scatter
    eng.set_order_mode("host")
    assert np.array_equal(eng.wait(eng.submit_batch(src, off, lens)), want)
    assert order_launches(eng) == 2  # host mode: none


def test_block_counts_past_the_cap_take_the_host_route(eng):
    """One 300 KB message among 64 B ones: 4,687 block counts apart."""
    rng = np.random.default_rng(12)
    n = 2000
    lens = np.full(n, 64, dtype=np.uint32)
    lens[n // 2] = 300_000
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    src = rng.integers(0, 256, int(off[-1]) + int(lens[-1]), dtype=np.uint8)
    assert (300_000 + 72) // 64 - (64 + 72) // 64 + 1 > _lib.MIRSHA_ORDER_MAX_BINS
    eng.set_order_mode("device")
    eng.set_timing(True)
    eng.reset_timing()
    got = eng.wait(eng.submit_batch(src, off, lens))
    assert order_launches(eng) == 0
    assert np.array_equal(got, oracle_py.hash_requests(src, off, lens))


def test_six_in_flight_mode_toggled_waited_out_of_order(eng):
    """More submissions than ring slots, every other one in device mode."""
    cases = [cycle(n, gap, seed=k) for k, (n, gap) in enumerate([(5000, 0), (1000, 5), (5000, 2000), (65, 0),
                                                                  (5000, 5), (1000, 0)])]
    tickets = []
    for k, (src, off, lens, _) in enumerate(cases):
        eng.set_order_mode("device" if k % 2 == 0 else "host")
        tickets.append(eng.submit_batch(src, off, lens))
    for k in (3, 0, 5, 1, 4, 2):
        assert np.array_equal(eng.wait(tickets[k]), cases[k][3]), k


def test_expect_submission_in_device_mode(eng):
    """Every other request carries an expectation, a few of them wrong: verdict
    bitmap, count and every kept row equal host mode's (unwritten rows keep
    the fill in both)."""
    n = 5000
    src, off, lens, want = cycle(n, 0)
    expected = [want[i].tobytes() if i % 2 == 0 else None for i in range(n)]
    wrong = [0, 64, 1998, 4998]
    for i in wrong:
        row = bytearray(expected[i])
        row[i % 32] ^= 0x40
        expected[i] = bytes(row)
    res = {}
    for pinned_out in (False, True):
        for mode in ("host", "device"):
            eng.set_order_mode(mode)
            out = eng.host_empty(32 * n).reshape(n, 32) if pinned_out else np.empty((n, 32), dtype=np.uint8)
            out[:] = 0xA5
            t = eng.submit_batch_expect(src, off, lens, expected, out=out)
            eng.wait(t)
            res[mode] = (t.mismatches.copy(), int(t._count[0]), t._bits.copy(), out.copy())
        h, d = res["host"], res["device"]
        assert d[0].tolist() == h[0].tolist() == wrong
        assert d[1] == h[1] == len(wrong)
        assert np.array_equal(d[2], h[2])
        assert np.array_equal(d[3], h[3])
        kept = np.array([i % 2 == 1 or i in wrong for i in range(n)])
        assert np.array_equal(d[3][kept], want[kept]) and bool((d[3][~kept] == 0xA5).all())


def test_validation_failure_in_device_mode_queues_nothing(eng):
    eng.set_order_mode("device")
    eng.set_timing(True)
    eng.reset_timing()
    src, off, lens, want = cycle(1000, 0)
    bad = off.copy()
    bad[57] = src.size  # request 57 outside the arena
    out = np.full((1000, 32), 0xA5, dtype=np.uint8)
    t = ctypes.c_uint64(0)
    before = eng.submit_batch(src, off, lens)
    rc = eng._lib.mirsha_submit_batch(eng.ctx, src.ctypes.data, src.size, bad.ctypes.data, lens.ctypes.data, 1000,
                                      out.ctypes.data, ctypes.byref(t))
    assert rc == _lib.MIRSHA_EINVAL and t.value == 0
    after = eng.submit_batch(src, off, lens)
    assert after.value == before.value + 1  # no ticket consumed
    assert np.array_equal(eng.wait(after), want) and np.array_equal(before.out, want)
    assert order_launches(eng) == 4  # the two good submissions only
    assert bool((out == 0xA5).all())


def test_invalid_modes(eng):
    for mode in (2, -1, 7):
        with pytest.raises(MirshaError) as e:
            eng.set_order_mode(mode)
        assert e.value.code == _lib.MIRSHA_EINVAL
        assert eng.order_mode == "host"
    with pytest.raises(ValueError):
        eng.set_order_mode("gpu")
    assert eng._lib.mirsha_ctx_set_order_mode(None, 1) == _lib.MIRSHA_EINVAL
