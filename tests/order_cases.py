"""Length sets for the device-built bucket order (mirsha_order.h), shared by
tests/test_order_host.py (a numpy restatement of the three passes) and
tests/test_gpu_order_device.py (the kernels): each case is (lengths, min_len,
max_len) with every length inside the bounds unless the case says otherwise."""
import numpy as np

CHUNK = 1024  # mirsha_order_plan's chunk for up to 1024 bins (the tests assert it)
SIZES = (1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
PATTERNS = ("alternating", "all_but_last", "ascending", "distinct64", "straddle")
EDGES = np.array([0, 55, 56, 119, 120, 183, 184], dtype=np.uint32)  # last / first length of 1, 2, 3, 4 blocks
MAX_BINS = 4096


def blocks(length):
    """SHA-256 blocks of a message: ceil((L + 9) / 64)."""
    return (np.asarray(length).astype(np.int64) + 72) >> 6


def longest_of(b):
    """The longest length of b blocks."""
    return (64 * np.asarray(b, dtype=np.int64) - 9).astype(np.uint32)


def pattern_blocks(name: str, n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.int64)
    if name == "alternating":  # two block counts
        return 2 + 3 * (i & 1)
    if name == "all_but_last":
        b = np.full(n, 3, dtype=np.int64)
        b[-1] = 7
        return b
    if name == "ascending":
        # Strictly ascending = a full reversal, up to one chunk.  Beyond that
        # it cannot be strict (strict means n bins, and a chunk holds at least
        # as many messages as there are bins), so the counts ascend in CHUNK
        # steps of equal width.
        return 1 + (i if n <= CHUNK else i * CHUNK // n)
    if name == "distinct64":  # 37 is odd: the 64 lanes of every wave step differ
        return 1 + (i * 37) % 64
    if name == "straddle":  # one block count on both sides of every chunk boundary, others around it
        b = 2 + i % 3
        for edge in range(CHUNK, n + CHUNK, CHUNK):
            b[max(0, edge - 40):edge + 40] = 4
        return b
    raise ValueError(name)


def pattern_case(name: str, n: int):
    lens = longest_of(pattern_blocks(name, n))
    return lens, int(lens.min()), int(lens.max())


def loguniform(n: int = 20_000, seed: int = 5):
    """Log-uniform 64 B - 64 KB lengths, both ends present."""
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(64.0), np.log(65536.0), n)).astype(np.uint32)
    lens[7], lens[n - 3] = 64, 65536
    return np.clip(lens, 64, 65536).astype(np.uint32), 64, 65536


def max_bins(n: int = 2 * MAX_BINS + 3, seed: int = 6):
    """Exactly MAX_BINS bins: one long length among short ones."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 56, n).astype(np.uint32)  # one block each
    lens[n // 3] = int(longest_of(MAX_BINS))
    return lens, 0, int(longest_of(MAX_BINS))


def clamped_order(lens, min_len: int, max_len: int) -> np.ndarray:
    """What the device builds for any lengths: stable by the clamped bin."""
    bmin, bmax = int(blocks(min_len)), int(blocks(max_len))
    bins = np.clip(bmax - blocks(lens), 0, bmax - bmin)
    return np.argsort(bins, kind="stable").astype(np.uint32)


def three_passes(lens, min_len: int, max_len: int, bins: int, chunk: int, n_chunks: int) -> np.ndarray:
    """The count, scan and scatter launches restated in numpy."""
    n = lens.size
    bmax = int(blocks(max_len))
    which = np.clip(bmax - blocks(lens), 0, bins - 1)
    counts = np.zeros((bins, n_chunks), dtype=np.int64)  # bin-major
    for c in range(n_chunks):
        counts[:, c] = np.bincount(which[c * chunk:(c + 1) * chunk], minlength=bins)
    flat = counts.reshape(-1)
    base = (np.cumsum(flat) - flat).reshape(bins, n_chunks)  # exclusive
    order = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    for c in range(n_chunks):
        seg = which[c * chunk:(c + 1) * chunk]
        by_bin = np.argsort(seg, kind="stable")  # index order inside a bin
        sb = seg[by_bin]
        rank = np.arange(seg.size) - np.searchsorted(sb, sb, side="left")
        order[base[sb, c] + rank] = c * chunk + by_bin
    return order
