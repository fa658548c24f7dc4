"""rt_ivf_topk_lists (csrc/ivf.hip): the probed-list scan reading CSR exclusion
lists of ORIGINAL positions, on the hand-made layout of test_gpu_ivf_kernels.py
— 16 lists over 3,000 rows, lengths 0, 1, 63, 64, 65, 255, 256, 257, 700, ...,
row_pos a random permutation, one list longer than a chunk.

Every comparison is np.array_equal on ids and on score bits against two
references: the C oracle restricted to the probed lists with the equivalent
bitmap (_ivf_ref.probed_lists_search), and kernels.ivf_topk with that bitmap.
LDS_CAP is the number of positions per query the scan stages in LDS
(include/rtrec_hip.h); longer CSR rows are searched in global memory."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _ivf_ref as ref
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
DT_IDS = ["f32", "f16", "bf16"]
NEG = -np.finfo(np.float32).max
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 100, 30, 200, 150, 90, 300, 469]
NLIST, N = len(LENGTHS), sum(LENGTHS)
EMPTY_LIST, LONG_LIST = 0, 8
CASES = [(dt, d) for dt in DTYPES for d in ((4, 132) if dt == F32 else (8, 136))]
CASE_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-d{d}" for dt, d in CASES]
LDS_CAP = 8960
NQ = 33


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    assert N == 3000
    chunks, rows_per_chunk, _ = kernels.ivf_topk_plan(1, NLIST, max(LENGTHS))
    assert LENGTHS[LONG_LIST] > rows_per_chunk and chunks > 1, "one list must span several chunks"
    return kernels


def _bits(t):
    """What the oracle takes for a tensor: (array, dtype_code)."""
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


@functools.lru_cache(maxsize=None)
def _layout(seed=0):
    """(offsets [17], row_pos [N] int32, assignment [N] by original position)."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    row_pos = rng.permutation(N).astype(np.int32)
    assignment = np.empty(N, np.int64)
    assignment[row_pos] = np.repeat(np.arange(NLIST), LENGTHS)
    return offsets, row_pos, assignment


@functools.lru_cache(maxsize=None)
def _case(dt, d, equal=False):
    """CPU tensors in ``dt``: queries [33, d], corpus x [N, d] in ORIGINAL order."""
    rng = np.random.default_rng(100 * d + DTYPES.index(dt))
    q = torch.from_numpy(rng.standard_normal((NQ, d)).astype(np.float32)).to(dt)
    x = rng.standard_normal((N, d)).astype(np.float32)
    if equal:
        x[:] = x[0]
    return q, torch.from_numpy(x).to(dt)


@functools.lru_cache(maxsize=None)
def _flat_oracle(dt, d):
    q, x = _case(dt, d)
    qa, code = _bits(q)
    return orc.flat_ip_search(qa, _bits(x)[0], 128, dtype_code=code, nthreads=16)


@functools.lru_cache(maxsize=None)
def _device(dt, d, equal=False):
    """(queries, stored rows, list offsets, row_pos) on the device."""
    q, x = _case(dt, d, equal)
    offsets, row_pos, _ = _layout()
    stored = x[torch.from_numpy(row_pos.astype(np.int64))].contiguous()
    return q.cuda(), stored.cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(row_pos).cuda()


def _probes(nq, nprobe, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(NLIST)[:nprobe] for _ in range(nq)]).astype(np.int64)


def _csr(lists):
    """(offsets int64 [n + 1], items int32) of per-row item sequences, kept as given."""
    offsets = np.zeros(len(lists) + 1, np.int64)
    offsets[1:] = np.cumsum([len(e) for e in lists])
    items = np.concatenate([np.asarray(e, np.int64) for e in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return offsets, items


def _mask(sources, nq):
    """bool [nq, N]: the union over the sources of each query's CSR row (the contract
    of RtExclusionLists: row rows[q] or q; a row outside the CSR and items outside
    the corpus exclude nothing)."""
    m = np.zeros((nq, N), bool)
    for offsets, items, rows in sources:
        n_rows = len(offsets) - 1
        for q in range(nq):
            r = int(rows[q]) if rows is not None else q
            if 0 <= r < n_rows:
                it = items[offsets[r]:offsets[r + 1]].astype(np.int64)
                m[q, it[(it >= 0) & (it < N)]] = True
    return m


def _to_device(sources):
    return [tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in src)
            for src in sources]


def _assert_equal(got, rs, ri, what=""):
    torch.cuda.synchronize()
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), what


def _check(K, dt, d, nq, k, probes, sources, equal=False, what=""):
    """The lists call against the oracle and against the bitmap kernel; returns the oracle's (scores, ids)."""
    q, x = _case(dt, d, equal)
    qd, stored, od, pd = _device(dt, d, equal)
    assignment = _layout()[2]
    qa, code = _bits(q[:nq])
    mask = _mask(sources, nq)
    bits = ref.bitmap_of_excluded(mask)
    rs, ri = ref.probed_lists_search(qa, _bits(x)[0], assignment, probes, k, exclude_bits=bits, dtype_code=code)
    assert not mask[np.arange(nq)[:, None], np.where(ri >= 0, ri, 0)][ri >= 0].any()   # the reference itself
    pr = torch.from_numpy(probes).cuda()
    qn = qd[:nq].contiguous()
    by_bits = K.ivf_topk(qn, stored, od, pd, pr, max(LENGTHS), k,
                         exclude_bits=torch.from_numpy(bits.view(np.int32)).cuda())
    _assert_equal(by_bits, rs, ri, what + " (bitmap kernel)")
    got = K.ivf_topk(qn, stored, od, pd, pr, max(LENGTHS), k, exclude_lists=_to_device(sources))
    _assert_equal(got, rs, ri, what + " (lists)")
    return rs, ri


def _standard_lists(dt, d):
    """33 CSR rows that hold every small case: empty, one item, positions 0 and
    N - 1, items >= nx, duplicates, lengths 1 / 63 / 64 / 65 drawn from the
    query's own unrestricted top-128 (so that they bite), longer random rows."""
    top = _flat_oracle(dt, d)[1]
    rng = np.random.default_rng(11)
    lists = []
    for q in range(NQ):
        kind = q % 11
        if kind == 0:
            e = []
        elif kind == 1:
            e = [top[q, 0]]
        elif kind == 2:
            e = [0, N - 1]
        elif kind == 3:
            e = [top[q, 1], N, N + 7, 2 ** 31 - 1]
        elif kind == 4:
            e = [0, top[q, 0], top[q, 0], top[q, 0], top[q, 2], top[q, 2], N - 1, N - 1, N + 3]
        elif kind in (5, 6, 7):
            e = rng.choice(top[q], (63, 64, 65)[kind - 5], replace=False)
        elif kind == 8:
            e = rng.integers(0, N, 300)     # duplicates
        elif kind == 9:
            e = rng.integers(0, N, 1500)
        else:
            e = rng.choice(top[q], 100, replace=False)
        lists.append(np.sort(np.asarray(e, np.int64)))
    return lists


@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_grid(K, dt, d):
    """nq x k x nprobe with one source holding every small case per query."""
    lists = _standard_lists(dt, d)
    for nq in (1, 8, 33):
        src = _csr(lists[:nq]) + (None,)
        for nprobe in (1, 4, NLIST):
            probes = _probes(nq, nprobe)
            for k in (1, 10, 128):
                _check(K, dt, d, nq, k, probes, [src], what=f"nq={nq} k={k} nprobe={nprobe}")
    # the one-item query of the grid loses exactly its best row
    rs, ri = _check(K, dt, d, 2, 10, _probes(2, NLIST), [_csr(lists[:2]) + (None,)])
    assert ri[1, 0] == _flat_oracle(dt, d)[1][1, 1]


@pytest.mark.parametrize("dt,d", [(F32, 4), (F16, 136)], ids=["f32-d4", "f16-d136"])
@pytest.mark.parametrize("tiles", [0, 4], ids=["chunk-default", "chunk-4-tiles"])
def test_lds_cap_boundary(K, dt, d, tiles):
    """CSR rows just below, at and just above the LDS cap and several times the cap
    (positions drawn from 3,000 with duplicates): both tiers and the boundary;
    two sources whose sum crosses the cap while each fits. With the chunk floor
    at 4 tiles a block walks several tiles, the next tile's loads in flight
    under the search."""
    rng = np.random.default_rng(5)
    lens = [LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 4 * LDS_CAP + 3]
    one = _csr([np.sort(rng.integers(0, N, n)) for n in lens]) + (None,)
    half = LDS_CAP // 2
    a = _csr([np.sort(rng.integers(0, N // 2, n)) for n in (half, half, half + 1, LDS_CAP)]) + (None,)
    b = _csr([np.sort(rng.integers(N // 3, N, n)) for n in (half - 1, half, half, 1)]) + (None,)
    try:
        K.ivf_topk_tuning(tiles)
        for nprobe in (4, NLIST):
            probes = _probes(4, nprobe, seed=3)
            _check(K, dt, d, 4, 128, probes, [one], what=f"one source nprobe={nprobe}")
            _check(K, dt, d, 4, 128, probes, [a, b], what=f"two sources nprobe={nprobe}")
    finally:
        K.ivf_topk_tuning(0)


@pytest.mark.parametrize("dt,d", [(F32, 132), (BF16, 8)], ids=["f32-d132", "bf16-d8"])
def test_two_sources_and_rows(K, dt, d):
    """Two sources whose rows overlap; the second through ``rows`` with a repeated
    row, -1 and n_rows (both: nothing excluded)."""
    lists = _standard_lists(dt, d)
    top = _flat_oracle(dt, d)[1]
    nq = 8
    a = _csr(lists[:nq]) + (None,)
    shared = [np.sort(top[0, :40]), np.arange(0, N, 2), np.sort(np.concatenate([top[3, :10], top[5, :10]]))]
    rows = np.array([0, 1, 1, 2, -1, 2, 3, 1], np.int64)   # 3 == n_rows
    b = _csr(shared) + (rows,)
    probes = _probes(nq, NLIST)
    for k in (10, 128):
        rs, ri = _check(K, dt, d, nq, k, probes, [a, b], what=f"k={k}")
        assert not np.isin(ri[0], top[0, :40]).any()
        assert (ri[1][ri[1] >= 0] % 2 == 1).all() and (ri[2][ri[2] >= 0] % 2 == 1).all()
    _check(K, dt, d, nq, 10, _probes(nq, 4), [b], what="rows only")
    # rows longer than the call: the first nq entries are used
    _check(K, dt, d, 3, 10, _probes(3, 4), [b], what="rows longer than nq")


def test_whole_list_and_everything_excluded(K):
    """A CSR row holding every row of one probed list: that list contributes
    nothing. A row holding every position: every slot is a pad."""
    dt, d, k, nq = F32, 4, 128, 3
    assignment = _layout()[2]
    probes = np.array([[LONG_LIST, 5, 2], [7, LONG_LIST, 3], [4, 6, LONG_LIST]], np.int64)
    long_rows = np.nonzero(assignment == LONG_LIST)[0]
    src = _csr([long_rows, np.union1d(long_rows, np.arange(0, N, 3)), long_rows]) + (None,)
    rs, ri = _check(K, dt, d, nq, k, probes, [src])
    assert not np.isin(ri, long_rows).any()
    everything = _csr([np.arange(N)]) + (np.zeros(nq, np.int64),)
    rs, ri = _check(K, dt, d, nq, k, probes, [everything])
    assert (ri == -1).all() and (rs == NEG).all()
    # two sources that cover the corpus together
    lo = _csr([np.arange(N // 2)]) + (np.zeros(nq, np.int64),)
    hi = _csr([np.arange(N // 2, N)] * nq) + (None,)
    rs, ri = _check(K, dt, d, nq, k, probes, [lo, hi])
    assert (ri == -1).all()


@pytest.mark.parametrize("tiles", [0, 4], ids=["chunk-default", "chunk-4-tiles"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_all_equal_rows(K, dt, tiles):
    """All rows equal: the result is the positions in ascending order without the
    excluded ones, which sit in the middle of the tie order."""
    d, nq = 32, 4
    skip = [np.array([3, 4, 5, 64, 100, 101, 102, 127]), np.zeros(0, np.int64), np.arange(0, 200, 2),
            np.arange(1, 120)]
    src = _csr(skip) + (None,)
    try:
        K.ivf_topk_tuning(tiles)
        for k in (10, 128):
            rs, ri = _check(K, dt, d, nq, k, _probes(nq, NLIST, seed=2), [src], equal=True, what=f"k={k}")
            for q in range(nq):
                assert np.array_equal(ri[q], np.setdiff1d(np.arange(N), skip[q])[:k])
    finally:
        K.ivf_topk_tuning(0)


def test_no_lists_is_the_plain_scan(K):
    """n_lists == 0 (the C entry point directly, and the wrapper with a source that
    has no items): rt_ivf_topk without a bitmap, bit for bit."""
    native = K.native
    dt, d, k, nq = F16, 8, 10, 8
    qd, stored, od, pd = _device(dt, d)
    probes = torch.from_numpy(_probes(nq, 4)).cuda()
    qn = qd[:nq].contiguous()
    plain = K.ivf_topk(qn, stored, od, pd, probes, max(LENGTHS), k)
    empty = (torch.zeros(nq + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    got = K.ivf_topk(qn, stored, od, pd, probes, max(LENGTHS), k, exclude_lists=empty)
    s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(native.lib().rt_ivf_topk_workspace_bytes(nq, 4, max(LENGTHS), k), dtype=torch.uint8,
                     device="cuda")
    native.call("rt_ivf_topk_lists", native.ptr(qn), nq, native.ptr(stored), N, d, native.dtype_code(dt),
                native.ptr(od), NLIST, native.ptr(pd), native.ptr(probes), 4, max(LENGTHS), k,
                ctypes.POINTER(native.ExclusionLists)(), 0, native.ptr(s), native.ptr(i), native.ptr(ws),
                ws.numel(), native.stream_of(qn))
    torch.cuda.synchronize()
    for other in (got, (s, i)):
        assert torch.equal(other[1], plain[1])
        assert torch.equal(other[0].view(torch.int32), plain[0].view(torch.int32))


def test_query_chunks_of_the_wrapper(K):
    """2 x 32,768 + 5 queries (three rt_ivf_topk_lists calls): with ``rows`` each
    chunk takes its slice of them, without them query a + q still uses CSR row
    a + q. Against the bitmap kernel."""
    dt, d, k = F32, 4, 1
    nq = 2 * K.IVF_QUERY_CHUNK + 5
    _, stored, od, pd = _device(dt, d)
    rng = np.random.default_rng(9)
    qd = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).cuda()
    probes_np = rng.integers(0, NLIST, (nq, 1)).astype(np.int64)
    probes = torch.from_numpy(probes_np).cuda()
    best = K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k)[1].cpu().numpy()[:, 0]

    def by_bits(mask):
        bits = torch.from_numpy(ref.bitmap_of_excluded(mask).view(np.int32)).cuda()
        return K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k, exclude_bits=bits)

    # without rows: query q skips its own best row (two in three queries; the CSR ends 3 rows early)
    n_rows = nq - 3
    has = (np.arange(n_rows) % 3 != 0) & (best[:n_rows] >= 0)
    offsets = np.zeros(n_rows + 1, np.int64)
    offsets[1:] = np.cumsum(has)
    items = best[:n_rows][has].astype(np.int32)
    mask = np.zeros((nq, N), bool)
    mask[np.nonzero(has)[0], items] = True
    want = by_bits(mask)
    got = K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k,
                     exclude_lists=(torch.from_numpy(offsets).cuda(), torch.from_numpy(items).cuda()))
    torch.cuda.synchronize()
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    changed = got[1].cpu().numpy()[:, 0] != best
    assert changed[:n_rows][has].all() and not changed[n_rows:].any() and not changed[:n_rows][~has].any()
    # the chunk boundaries themselves
    for q in (K.IVF_QUERY_CHUNK - 1, K.IVF_QUERY_CHUNK, K.IVF_QUERY_CHUNK + 1, 2 * K.IVF_QUERY_CHUNK + 1):
        assert changed[q] == has[q]

    # with rows: 7 CSR rows of 1,500 positions, rows[q] in -1..7 (7 == n_rows)
    shared = [np.sort(rng.integers(0, N, 1500)) for _ in range(7)]
    so, si = _csr(shared)
    rows = (np.arange(nq) * 5 % 9 - 1).astype(np.int64)
    mask = _mask([(so, si, rows)], nq)
    want = by_bits(mask)
    got = K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k,
                     exclude_lists=(torch.from_numpy(so).cuda(), torch.from_numpy(si).cuda(),
                                    torch.from_numpy(rows).cuda()))
    torch.cuda.synchronize()
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert (got[1].cpu().numpy()[:, 0] != best).any()
