"""The category filter in the scans: rt_flatip_topk_online_tags,
rt_ivf_topk_tags and rt_tag_filter_bitmap against the existing oracles.

A filter is the exclusion bitmap of the ineligible items (_tag_filter_ref), so
every expectation is oracle.flat_ip.flat_ip_search(..., exclude_bits=...) or
_ivf_ref.probed_lists_search(..., exclude_bits=...), and every comparison is
bit for bit on scores and ids."""
import functools

import numpy as np
import pytest
import torch

import _ivf_ref as ref
import _ordered_corpora as oc
import _tag_filter_ref as tref
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
NEG = -np.finfo(np.float32).max
BIT63 = np.uint64(1) << np.uint64(63)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


def _bits(t):
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


def _dev(words):
    """uint64 words -> int64 device tensor of the same bits."""
    return torch.from_numpy(tref.as_i64(words).copy()).cuda()


def _filter(tags, any_of, none_of):
    return (_dev(tags), None if any_of is None else _dev(any_of), None if none_of is None else _dev(none_of))


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(e) for e in lists], out=off[1:])
    items = np.concatenate([np.asarray(e, np.int32) for e in lists]) if off[-1] else np.zeros(0, np.int32)
    return (torch.from_numpy(off).cuda(), torch.from_numpy(items.astype(np.int32)).cuda())


def _excluded_mask(lists, n):
    m = np.zeros((len(lists), n), bool)
    for q, e in enumerate(lists):
        m[q, np.asarray(e, np.int64)] = True
    return m


def _flat_oracle(q_t, x_t, k, bits):
    qa, code = _bits(q_t)
    xa, _ = _bits(x_t)
    return orc.flat_ip_search(qa, xa, k, exclude_bits=bits, dtype_code=code, nthreads=16)


def _assert_equal(got, rs, ri, what=""):
    torch.cuda.synchronize()
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs, rs), what


# ---- Flat online -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat_case(nx):
    rows, queries = ref.clustered_corpus()
    return torch.from_numpy(queries[:8].copy()), torch.from_numpy(rows[:nx].copy())


@DTYPES
@pytest.mark.parametrize("nx", [8192, 7777])
@pytest.mark.parametrize("nq", [1, 8])
def test_flat_online_filter(K, dtype, nx, nq):
    """Per-query masks all different; k = 1, 20, 128 over one upload."""
    q32, x32 = _flat_case(nx)
    qt, xt = q32[:nq].to(dtype), x32.to(dtype)
    tags = tref.fixture_tags(nx)
    any_of, none_of = tref.fixture_masks(8)
    any_of, none_of = any_of[8 - nq:], none_of[8 - nq:]   # nq = 1: query 7's masks, not the trivial first pair
    bits = tref.filter_bits(tags, any_of, none_of)
    qd, xd, flt = qt.cuda(), xt.cuda(), _filter(tags, any_of, none_of)
    for k in (1, 20, 128):
        rs, ri = _flat_oracle(qt, xt, k, bits)
        assert (ri >= 0).all()
        _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=flt), rs, ri, f"{dtype} nx={nx} nq={nq} k={k}")


@DTYPES
def test_flat_online_special_masks(K, dtype):
    q32, x32 = _flat_case(8192)
    qt, xt = q32.to(dtype), x32.to(dtype)
    qd, xd = qt.cuda(), xt.cuda()
    tags = tref.fixture_tags(8192)
    k = 20
    zero = np.zeros(8, np.uint64)
    # masks that select nothing: a category no item has; any_of == none_of
    for any_of, none_of in ((np.full(8, 1 << 40, np.uint64), zero), (np.full(8, 1, np.uint64), np.full(8, 1, np.uint64))):
        s, i = K.flatip_topk_online(qd, xd, k, tag_filter=_filter(tags, any_of, none_of))
        torch.cuda.synchronize()
        assert (i.cpu().numpy() == -1).all() and (s.cpu().numpy() == NEG).all()
    # bit 63: its 6 items, then pads
    any63 = np.full(8, BIT63, np.uint64)
    rs, ri = _flat_oracle(qt, xt, k, tref.filter_bits(tags, any63, zero))
    assert ((ri >= 0).sum(axis=1) == 6).all() and (ri[:, 6:] == -1).all()
    _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=_filter(tags, any63, zero)), rs, ri, "bit 63")
    # any_of = none_of = 0 (given, or NULL): the unfiltered call's bits
    plain = K.flatip_topk_online(qd, xd, k)
    rs, ri = plain[0].cpu().numpy(), plain[1].cpu().numpy()
    _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=_filter(tags, zero, zero)), rs, ri, "zero masks")
    _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=_filter(tags, None, None)), rs, ri, "NULL masks")
    # only none_of given
    none_of = tref.fixture_masks(8)[1]
    rs, ri = _flat_oracle(qt, xt, k, tref.filter_bits(tags, zero, none_of))
    _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=_filter(tags, None, none_of)), rs, ri, "none_of only")


@DTYPES
def test_flat_online_filter_with_two_list_sources(K, dtype):
    """Each query's exclusion lists hold its own filtered top-k (source 0) and its
    neighbour's (source 1): the result is the next eligible rows."""
    nx, k = 7777, 50
    q32, x32 = _flat_case(nx)
    qt, xt = q32.to(dtype), x32.to(dtype)
    tags = tref.fixture_tags(nx)
    any_of, none_of = tref.fixture_masks(8)
    fbits = tref.filter_bits(tags, any_of, none_of)
    _, top = _flat_oracle(qt, xt, k, fbits)
    own = [np.sort(top[q]) for q in range(8)]
    other = [np.sort(top[(q + 1) % 8]) for q in range(8)]
    both = _excluded_mask(own, nx) | _excluded_mask(other, nx)
    rs, ri = _flat_oracle(qt, xt, k, fbits | ref.bitmap_of_excluded(both))
    for q in range(8):
        assert not set(ri[q].tolist()) & (set(own[q].tolist()) | set(other[q].tolist()))
    got = K.flatip_topk_online(qt.cuda(), xt.cuda(), k, exclude_lists=[_csr(own), _csr(other)],
                               tag_filter=_filter(tags, any_of, none_of))
    _assert_equal(got, rs, ri, f"{dtype}")


@functools.lru_cache(maxsize=None)
def _compaction_case():
    """524,251 rows whose score ascends inside every block of 1,024 rows (the
    scan's rows per block here: four tiles): every row passes the running
    threshold, so a block's candidate buffer goes above kRoom = 192 and is
    compacted. Scores repeat from block to block: ties, resolved by position."""
    from rtrec_amd import kernels
    nx, d = 524_251, 32
    blocks, rpb = kernels.flatip_topk_online_plan(8, nx, d, F32, 128)
    assert (blocks, rpb) == (512, 1024) and nx % 256 != 0
    ranks = np.zeros((nx, 2), np.int64)
    ranks[:, 0] = np.arange(nx) % 1024
    ranks[:, 1] = 1023 - np.arange(nx) % 1024
    x = oc.encode(ranks, d)
    q = oc.queries([(0, 1.0), (0, 2.0), (1, 1.0), (0, 4.0), (0, 1.0), (1, 2.0), (0, 2.0), (0, 1.0)], d)
    return torch.from_numpy(q), torch.from_numpy(x)


@DTYPES
def test_flat_online_compaction_under_filter(K, dtype):
    """The filter is a tag that every other row carries: 128 of a tile's 256 rows are
    eligible, the buffer passes kRoom in the second tile and the third starts with
    a compaction. An ineligible row counted or kept by it changes the result."""
    q32, x32 = _compaction_case()
    qt, xt = q32.to(dtype), x32.to(dtype)
    nx = xt.shape[0]
    tags = np.where(np.arange(nx) % 2 == 0, 1, 2).astype(np.uint64)
    any_of = np.array([1, 2, 1, 0, 0, 2, 0, 3], np.uint64)
    none_of = np.array([0, 0, 0, 1, 2, 0, 0, 0], np.uint64)
    bits = tref.filter_bits(tags, any_of, none_of)
    qd, xd, flt = qt.cuda(), xt.cuda(), _filter(tags, any_of, none_of)
    for k in (20, 128):
        rs, ri = _flat_oracle(qt, xt, k, bits)
        _assert_equal(K.flatip_topk_online(qd, xd, k, tag_filter=flt), rs, ri, f"{dtype} k={k}")


def test_flat_online_duplicate_rows_tie_rule(K):
    """A block of 96 identical rows (the best for query 0) with different tags:
    the lower-position-wins rule applies among the ELIGIBLE rows only."""
    q32, x32 = _flat_case(8192)
    x = x32.clone()
    x[1000:1096] = q32[0]
    tags = tref.fixture_tags(8192).copy()
    tags[1000:1096] = np.where(np.arange(96) % 3 == 1, 1 << 20, 1 << 21).astype(np.uint64)
    any_of = np.full(8, 1 << 20, np.uint64)
    none_of = np.zeros(8, np.uint64)
    rs, ri = _flat_oracle(q32, x, 20, tref.filter_bits(tags, any_of, none_of))
    assert ri[0].tolist() == list(range(1001, 1096, 3))[:20] and len(set(rs[0].tolist())) == 1
    _assert_equal(K.flatip_topk_online(q32.cuda(), x.cuda(), 20, tag_filter=_filter(tags, any_of, none_of)), rs, ri)


# ---- IVF scan ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ivf_layout(slack=0):
    """The fixture's lists as rt_ivf_topk stores them (host arrays): rows
    list-contiguous in position order inside a list; ``slack`` empty slots
    (row_pos = -1, rows of NaN-free garbage) behind every list."""
    f = tref.ivf_fixture()
    a = f["assignment"]
    order = np.argsort(a, kind="stable")
    counts = np.bincount(a, minlength=tref.NLIST)
    cap = counts + slack
    off = np.zeros(tref.NLIST + 1, np.int64)
    np.cumsum(cap, out=off[1:])
    total = int(off[-1])
    rows = np.full((total, f["rows"].shape[1]), 9.0, np.float32)   # an empty slot would score high
    row_pos = np.full(total, -1, np.int32)
    src = 0
    for l in range(tref.NLIST):
        n = int(counts[l])
        rows[off[l]:off[l] + n] = f["rows"][order[src:src + n]]
        row_pos[off[l]:off[l] + n] = order[src:src + n]
        src += n
    return rows, off, row_pos, counts.astype(np.int64), int(cap.max())


def _ivf_call(K, dtype, nprobe, k, slack, exclude_lists=None, flt=None):
    f = tref.ivf_fixture()
    rows, off, row_pos, counts, max_cap = _ivf_layout(slack)
    kw = {}
    if slack:
        # two of a list's empty slots count as live: the scan reads their row_pos = -1
        kw = dict(list_len=torch.from_numpy(counts + 2).cuda(), n_pos=len(f["rows"]))
    return K.ivf_topk(torch.from_numpy(f["queries"].copy()).to(dtype).cuda(), torch.from_numpy(rows).to(dtype).cuda(),
                      torch.from_numpy(off).cuda(), torch.from_numpy(row_pos).cuda(),
                      torch.from_numpy(tref.fixture_probes(nprobe).copy()).cuda(), max_cap, k,
                      exclude_lists=exclude_lists, tag_filter=flt, **kw)


def _ivf_oracle(dtype, nprobe, k, bits):
    f = tref.ivf_fixture()
    qa, code = _bits(torch.from_numpy(f["queries"].copy()).to(dtype))
    xa, _ = _bits(torch.from_numpy(f["rows"].copy()).to(dtype))
    return ref.probed_lists_search(qa, xa, f["assignment"], tref.fixture_probes(nprobe), k, exclude_bits=bits,
                                   dtype_code=code)


@DTYPES
@pytest.mark.parametrize("nprobe,k", [(4, 20), (4, 100), (64, 100)])
@pytest.mark.parametrize("slack", [0, 5], ids=["dense", "slack"])
def test_ivf_filter(K, dtype, nprobe, k, slack):
    """Without and with exclusion lists (each query's own filtered top-10), over
    lists without slack (list_len == NULL) and with slack, whose empty slots hold
    row_pos = -1 and rows that would outscore everything; two of them per list are
    inside list_len, so the scan meets the -1: dropped, and no tag gathered for it."""
    f = tref.ivf_fixture()
    flt = _filter(f["tags"], f["any_of"], f["none_of"])
    fbits = tref.filter_bits(f["tags"], f["any_of"], f["none_of"])
    rs, ri = _ivf_oracle(dtype, nprobe, k, fbits)
    pads = int((ri[:, -1] < 0).sum())
    assert pads == {(4, 20): 1, (4, 100): 256, (64, 100): 0}[(nprobe, k)]
    _assert_equal(_ivf_call(K, dtype, nprobe, k, slack, flt=flt), rs, ri, "filter")
    own = [np.sort(ri[q][:10][ri[q][:10] >= 0]) for q in range(len(ri))]
    rs2, ri2 = _ivf_oracle(dtype, nprobe, k, fbits | ref.bitmap_of_excluded(_excluded_mask(own, len(f["rows"]))))
    _assert_equal(_ivf_call(K, dtype, nprobe, k, slack, exclude_lists=_csr(own), flt=flt), rs2, ri2, "filter + lists")


def test_ivf_filter_null_is_the_lists_entry_and_all_lists_is_flat(K):
    f = tref.ivf_fixture()
    k = 100
    # zero masks: the unfiltered call's bits
    plain = _ivf_call(K, F32, 4, k, 0)
    zero = np.zeros(len(f["queries"]), np.uint64)
    _assert_equal(_ivf_call(K, F32, 4, k, 0, flt=_filter(f["tags"], zero, None)), plain[0].cpu().numpy(),
                  plain[1].cpu().numpy(), "zero masks")
    # nprobe = nlist: the filtered Flat result over the corpus in original order
    fbits = tref.filter_bits(f["tags"], f["any_of"], f["none_of"])
    rs, ri = orc.flat_ip_search(f["queries"], f["rows"], k, exclude_bits=fbits, nthreads=16)
    _assert_equal(_ivf_call(K, F32, 64, k, 5, flt=_filter(f["tags"], f["any_of"], f["none_of"])), rs, ri, "all lists")
    for a in (0, 248):
        flat = K.flatip_topk_online(torch.from_numpy(f["queries"][a:a + 8].copy()).cuda(),
                                    torch.from_numpy(f["rows"].copy()).cuda(), k,
                                    tag_filter=_filter(f["tags"], f["any_of"][a:a + 8], f["none_of"][a:a + 8]))
        _assert_equal(flat, rs[a:a + 8], ri[a:a + 8], f"flat online {a}")


# ---- rt_tag_filter_bitmap -------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 300])
@pytest.mark.parametrize("n_items", [8192, 1000, 31])
def test_tag_filter_bitmap(K, nq, n_items):
    tags = tref.fixture_tags(8192)[:n_items].copy()
    any_of, none_of = tref.fixture_masks(nq)
    any_of, none_of = any_of.copy(), none_of.copy()
    if nq > 2:
        any_of[1] = 0            # none_of alone
        any_of[2] = none_of[2] = 0   # nothing filtered
    want = tref.filter_bits(tags, any_of, none_of)
    words = want.shape[1]
    t, a, n = _filter(tags, any_of, none_of)
    got = K.tag_filter_bitmap(t, a, n, nq)
    torch.cuda.synchronize()
    assert got.shape == (nq, words) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    # overwrite: a dirty buffer, wider than needed — every word of a row written, pad bits zero
    out = torch.full((nq, words + 3), -1, dtype=torch.int32, device="cuda")
    K.tag_filter_bitmap(t, a, n, nq, n_items=n_items, out=out)
    full = np.zeros((nq, words + 3), np.uint32)
    full[:, :words] = want
    assert np.array_equal(out.cpu().numpy().view(np.uint32), full)
    # accumulate: OR onto another exclusion bitmap
    rng = np.random.default_rng(3)
    other = rng.integers(0, 1 << 32, size=(nq, words), dtype=np.uint64).astype(np.uint32)
    out = torch.from_numpy(other.view(np.int32).copy()).cuda()
    K.tag_filter_bitmap(t, a, n, nq, out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), other | want)
    # NULL masks: nothing filtered
    got = K.tag_filter_bitmap(t, None, None, nq)
    assert not got.cpu().numpy().any()


def test_bitmap_route_equals_native_filter(K):
    """The route of the paths without a native filter: rt_tag_filter_bitmap
    accumulated onto an exclusion bitmap, then rt_flatip_topk — the same lists as
    the scan's own filter with the same exclusions as lists."""
    q32, x32 = _flat_case(7777)
    nx, k = 7777, 20
    tags = tref.fixture_tags(nx)
    any_of, none_of = tref.fixture_masks(8)
    excl = [np.arange(q, nx, 9) for q in range(8)]
    bits = torch.from_numpy(ref.bitmap_of_excluded(_excluded_mask(excl, nx)).view(np.int32).copy()).cuda()
    t, a, n = _filter(tags, any_of, none_of)
    K.tag_filter_bitmap(t, a, n, 8, out=bits, accumulate=True)
    qd, xd = q32.cuda(), x32.cuda()
    via_bitmap = K.flatip_topk(qd, xd, k, exclude_bits=bits)
    native = K.flatip_topk_online(qd, xd, k, exclude_lists=_csr(excl), tag_filter=(t, a, n))
    _assert_equal(native, via_bitmap[0].cpu().numpy(), via_bitmap[1].cpu().numpy())
