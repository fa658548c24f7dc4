"""rt_rows_compact / rt_scatter_rows on the device, bit for bit (rows are int32
words): the compaction at the word edges (31/32/33), the segment edges
(2,047/2,048/2,049; a segment is 2,048 rows = 64 bitmap words) and with the
carry across three segments (3 * 2,048 + 5), for 16-, 256- and 1,040-byte rows
(1,040 = the d = 256 L2 row) and every keep pattern; the scatter with
out-of-range positions counted and skipped."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEG = 2048
N_ROWS = (1, 31, 32, 33, SEG - 1, SEG, SEG + 1, 3 * SEG + 5)
ROW_BYTES = (16, 256, 1040)
PATTERNS = ("all", "none", "first", "last", "alternating", "middle_segment", "p0.5", "p0.999")
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


def _keep(pattern, n, rng):
    keep = np.zeros(n, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern == "middle_segment":  # one whole segment cleared (the middle third where there is no such segment)
        keep[:] = True
        lo, hi = (SEG, 2 * SEG) if n > 2 * SEG else (n // 3, 2 * n // 3)
        keep[lo:hi] = False
    elif pattern.startswith("p"):
        keep = rng.random(n) < float(pattern[1:])
    return keep


def _bits(keep, extra_words=2):
    """Bit j of word w = row 32w + j; the last word's bits beyond n_rows and
    ``extra_words`` further words are set: garbage the kernels must ignore."""
    n = keep.size
    padded = np.ones((-(-n // 32) + extra_words) * 32, dtype=bool)
    padded[:n] = keep
    return torch.from_numpy(np.packbits(padded, bitorder="little").view("<u4").view(np.int32).copy()).cuda()


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_compact_is_stable_and_exact(K, row_bytes):
    rng = np.random.default_rng(row_bytes)
    g = torch.Generator(device="cuda").manual_seed(row_bytes)
    for n in N_ROWS:
        src = torch.randint(-2**31, 2**31 - 1, (n, row_bytes // 4), generator=g, device="cuda", dtype=torch.int32)
        src0 = src.clone()
        for pattern in PATTERNS:
            keep = _keep(pattern, n, rng)
            dst = torch.full((n + 3, row_bytes // 4), SENTINEL, dtype=torch.int32, device="cuda")
            n_kept = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            assert K.rows_compact(src, _bits(keep), dst, n_kept) is n_kept
            want = int(keep.sum())
            what = (n, row_bytes, pattern)
            assert int(n_kept.item()) == want, what
            assert torch.equal(dst[:want], src0[torch.from_numpy(np.flatnonzero(keep)).cuda()]), what
            assert bool((dst[want:] == SENTINEL).all()), what     # rows from n_kept on: untouched
            assert torch.equal(src, src0), what                   # out of place


def test_compact_of_no_rows_writes_zero(K):
    src = torch.empty((0, 64), dtype=torch.int32, device="cuda")
    dst = torch.full((4, 64), SENTINEL, dtype=torch.int32, device="cuda")
    n_kept = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    K.rows_compact(src, torch.empty(0, dtype=torch.int32, device="cuda"), dst, n_kept)
    assert int(n_kept.item()) == 0 and bool((dst == SENTINEL).all())


def test_compact_refuses_what_the_abi_refuses(K):
    from rtrec_amd import native
    src = torch.zeros((100, 64), dtype=torch.int32, device="cuda")
    bits = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(native.RTError):      # dst_rows < n_rows
        K.rows_compact(src, bits, torch.zeros((99, 64), dtype=torch.int32, device="cuda"))
    with pytest.raises(native.RTError):      # in place
        K.rows_compact(src, bits, src)
    with pytest.raises(native.RTError):      # short bitmap
        K.rows_compact(src, bits[:3], torch.zeros((100, 64), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):          # 24-byte rows
        K.rows_compact(src[:, :6].contiguous(), bits, torch.zeros((100, 6), dtype=torch.int32, device="cuda"))


def test_compact_past_4_gib(K):
    """Source and destination byte offsets beyond 2^32 (4,400,000 rows of 1,040
    bytes = 4.58 GB, 97 % kept = 4.44 GB): the 64-bit vector offsets of the move
    kernel. Checked on the device; a second or two."""
    n, row_bytes = 4_400_000, 1040
    assert n * row_bytes > 2**32 and int(0.96 * n) * row_bytes > 2**32
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randint(-2**31, 2**31 - 1, (n, row_bytes // 4), generator=g, device="cuda", dtype=torch.int32)
    keep = np.random.default_rng(5).random(n) < 0.97
    keep[-1] = True
    dst = torch.full((n, row_bytes // 4), SENTINEL, dtype=torch.int32, device="cuda")
    n_kept = K.rows_compact(src, _bits(keep), dst)
    want = int(keep.sum())
    assert want * row_bytes > 2**32
    assert int(n_kept.item()) == want
    idx = torch.from_numpy(np.flatnonzero(keep)).cuda()
    for lo in range(0, want, 1 << 20):       # in slices: no second 4 GB copy
        hi = min(want, lo + (1 << 20))
        assert torch.equal(dst[lo:hi], src[idx[lo:hi]]), lo
    assert bool((dst[want:] == SENTINEL).all())


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("n", [1, 3, 257])
def test_scatter_overwrites_exactly_the_named_rows(K, n, row_bytes):
    rows = 1000
    rng = np.random.default_rng(n * 7 + row_bytes)
    g = torch.Generator(device="cuda").manual_seed(n)
    dst = torch.randint(-2**31, 2**31 - 1, (rows, row_bytes // 4), generator=g, device="cuda", dtype=torch.int32)
    dst0 = dst.clone()
    # a random permutation prefix that includes 0 and 999, plus -1 and 1,000 (out of range)
    perm = [p for p in rng.permutation(rows).tolist() if p not in (0, rows - 1)]
    pos = ([0, rows - 1] + perm)[:n] if n > 1 else [0]
    if n == 1:
        pos_cases = [[0], [rows - 1]]
    else:
        pos_cases = [list(rng.permutation(pos))]
    for pos in pos_cases:
        dst.copy_(dst0)
        full = [-1] + list(pos) + [rows]
        src = torch.randint(-2**31, 2**31 - 1, (len(full), row_bytes // 4), generator=g, device="cuda",
                            dtype=torch.int32)
        src0 = src.clone()
        oob = torch.zeros(1, dtype=torch.int32, device="cuda")
        K.scatter_rows(src, torch.tensor(full, dtype=torch.int64, device="cuda"), dst, oob)
        assert int(oob.item()) == 2
        want = dst0.clone()
        want[torch.tensor(pos, device="cuda")] = src0[1:-1]
        assert torch.equal(dst, want), (n, row_bytes, pos[:4])
        assert torch.equal(src, src0)
    # no counter given: out-of-range positions are still skipped
    dst.copy_(dst0)
    K.scatter_rows(src0[:1], torch.tensor([rows], dtype=torch.int64, device="cuda"), dst)
    assert torch.equal(dst, dst0)
