"""The online (small-batch) Flat-IP top-K, rt_flatip_topk_online (csrc/
topk_online.hip): 1..8 queries, k <= 128, one streaming pass over the corpus.

Every comparison is np.array_equal on ids AND scores: fp32 scores are the
oracle's fmaf chain, and the 16-bit scans take the same chain over the widened
elements (every f16 x f16 and bf16 x bf16 product is exact in fp32), so random
f16 / bf16 corpora are bit-exact against oracle/flatip.c too — no tolerance,
no tie rule anywhere in this file.

Shapes are the smallest at which each path runs: 1 / 50 / 1,000 / 4,097 rows
(one block, k > rows, several blocks with a ragged last tile), the smallest
corpus at which the plan reports its largest grid (512 blocks, ragged last
block), and for the ordered corpora the largest corpus the exact-integer
encoding allows (2^18 ranks), which gives every block two 256-row tiles: the
first fills a candidate buffer past kRoom, the compaction check before the
second fires, and the second appends its full budget. Blocks of five tiles
(600,013 rows at d = 8: repeated compactions, a rising threshold, the strict
tie threshold followed by further tiles) run on random, few-valued and
all-equal rows."""
import functools

import numpy as np
import pytest
import torch

import _ordered_corpora as oc
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
DT_IDS = ["f32", "f16", "bf16"]
NEG = -np.finfo(np.float32).max


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


def _dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _bits(t):
    """What the oracle takes for a 16-bit tensor: (array, dtype_code)."""
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


def _oracle(q_t, x_t, k, **kw):
    qa, code = _bits(q_t)
    xa, _ = _bits(x_t)
    return orc.flat_ip_search(qa, xa, k, dtype_code=code, nthreads=16, **kw)


def _assert_equal(got, rs, ri, what=""):
    torch.cuda.synchronize()
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs, rs), what


@functools.lru_cache(maxsize=None)
def _largest_grid_nx():
    """The smallest corpus (minus a ragged tail) at which the plan reports its
    largest grid, read from the plan query at d = 32."""
    from rtrec_amd import kernels
    best, first = 0, 0
    for nx in (1 << s for s in range(8, 21)):
        blocks, _ = kernels.flatip_topk_online_plan(8, nx, 32, F32, 128)
        if blocks > best:
            best, first = blocks, nx
    assert best > 1
    nx = first - 37  # ragged last block and tile
    blocks, rpb = kernels.flatip_topk_online_plan(8, nx, 32, F32, 128)
    assert blocks == best and nx % rpb != 0
    return nx, blocks, rpb


# ---- 1. fp32, random: bit-exact against the oracle ---------------------------
@functools.lru_cache(maxsize=None)
def _random_case(nx, d, seed=0):
    rng = np.random.default_rng(1000 * d + nx + seed)
    q = rng.standard_normal((8, d)).astype(np.float32)
    x = rng.standard_normal((nx, d)).astype(np.float32)
    rs, ri = orc.flat_ip_search(q, x, 128, nthreads=16)
    for a in (q, x, rs, ri):
        a.setflags(write=False)
    return q, x, rs, ri


@pytest.mark.parametrize("d", [4, 100, 128, 256])
@pytest.mark.parametrize("nx", [1, 50, 1000, 4097])
def test_fp32_random_bit_exact(K, nx, d):
    """nq in {1, 3, 8} x k in {1, 10, 50, 128}; k > nx pads with (-FLT_MAX, -1).
    The rows are i.i.d. normal: no exact ties, so the oracle's top-128 of the 8
    queries holds every smaller case as a prefix."""
    q, x, rs, ri = _random_case(nx, d)
    xd = _dev(x)
    for nq in (1, 3, 8):
        qd = _dev(q[:nq])
        for k in (1, 10, 50, 128):
            got = K.flatip_topk_online(qd, xd, k)
            _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nx={nx} d={d} nq={nq} k={k}")
    if nx < 128:
        assert (ri[:, nx:] == -1).all() and (rs[:, nx:] == NEG).all()


def test_fp32_random_largest_grid(K):
    """512 blocks, the last one ragged: multi-block, the rank-major partial
    lists at their widest, the finish at one list per thread."""
    nx, blocks, rpb = _largest_grid_nx()
    assert blocks > 1
    q, x, rs, ri = _random_case(nx, 32)
    xd = _dev(x)
    for nq, k in ((1, 1), (1, 100), (3, 10), (8, 50), (8, 128)):
        got = K.flatip_topk_online(_dev(q[:nq]), xd, k)
        _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nx={nx} nq={nq} k={k}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("nx,d", [(1000, 128), (4097, 64), (50, 8), (4097, 256)])
def test_half_random_bit_exact(K, nx, d, dtype):
    """16-bit rows: the fp32 chain over the widened elements is the oracle's."""
    q, x, _, _ = _random_case(nx, d, seed=1)
    qt, xt = torch.from_numpy(q).to(dtype), torch.from_numpy(x).to(dtype)
    rs, ri = _oracle(qt, xt, 128)
    for nq, k in ((1, 50), (3, 128), (8, 100)):
        got = K.flatip_topk_online(qt[:nq].cuda(), xt.cuda(), k)
        _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nx={nx} d={d} nq={nq} k={k}")


# ---- 1b. many tiles per block ---------------------------------------------------
# 600,013 rows: rows_per_block = 1,172 = five 256-row tiles (the last ragged), so a
# block compacts several times with a rising threshold, as on a 10^6-row corpus
MANY_NX, MANY_D = 600_013, 8


def _many_plan():
    from rtrec_amd import kernels
    blocks, rpb = kernels.flatip_topk_online_plan(8, MANY_NX, MANY_D, F32, 128)
    assert rpb > 4 * 256 and blocks > 256
    return blocks, rpb


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_random_many_tiles_per_block(K, dtype):
    _many_plan()
    q, x, _, _ = _random_case(MANY_NX, MANY_D, seed=3)
    qt, xt = torch.from_numpy(q).to(dtype), torch.from_numpy(x).to(dtype)
    rs, ri = _oracle(qt, xt, 128)
    xd = xt.cuda()
    for nq, k in ((1, 100), (3, 10), (8, 128)):
        got = K.flatip_topk_online(qt[:nq].cuda(), xd, k)
        _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"many tiles {dtype} nq={nq} k={k}")


def test_few_distinct_scores_many_tiles_per_block(K):
    """Small-integer rows at d = 8: a few dozen distinct scores over 600,013
    rows, so every compaction resolves its bucket down into the ids and sets
    the strict tie threshold, and further tiles follow it. Exact in every
    dtype; the oracle breaks the ties by id."""
    _many_plan()
    rng = np.random.default_rng(21)
    x = rng.integers(-2, 3, (MANY_NX, MANY_D)).astype(np.float32)
    q = rng.integers(-2, 3, (8, MANY_D)).astype(np.float32)
    rs, ri = orc.flat_ip_search(q, x, 128, nthreads=16)
    for dtype in DTYPES:
        xd = _dev(x, dtype)
        for nq, k in ((1, 128), (8, 100)):
            got = K.flatip_topk_online(_dev(q[:nq], dtype), xd, k)
            _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"few scores {dtype} nq={nq} k={k}")


def test_identical_rows_many_tiles_per_block(K):
    """Every row equal, five tiles per block: ids 0..127 for every query."""
    _many_plan()
    k = 128
    x = np.full((MANY_NX, MANY_D), 0.5, np.float32)
    q = (np.arange(8 * MANY_D, dtype=np.float32).reshape(8, MANY_D) % 7 - 3.0) * 0.25
    want_s = np.repeat((q.astype(np.float64) @ x[0].astype(np.float64)).astype(np.float32)[:, None], k, axis=1)
    for dtype in (F32, F16):
        got = K.flatip_topk_online(_dev(q, dtype), _dev(x, dtype), k)
        _assert_equal(got, want_s, np.broadcast_to(np.arange(k), (8, k)), f"identical rows, many tiles {dtype}")


# ---- 2. ordered corpora -------------------------------------------------------
ORD_D = 16          # 5 groups of 3 dims; 32-byte f16 rows, 64-byte fp32 rows
# mixed +- scales over the five orderings (a negative scale reverses one)
ORD_PAIRS = ((0, 1.0), (0, -2.0), (1, 4.0), (2, 1.0), (3, 2.0), (3, -1.0), (4, 1.0), (2, -4.0))
# the largest corpus whose ranks (clustered_top: nx + 128 of them) fit 2^18: rows_per_block = 512
# = two tiles per block; and one with a single ragged-free 256-row tile per block
ORD_NX = (oc.MAX_RANK - 129, 100_003)


@functools.lru_cache(maxsize=None)
def _ordered(nx, k):
    from rtrec_amd import kernels
    blocks, rpb = kernels.flatip_topk_online_plan(8, nx, ORD_D, F32, k)
    assert blocks > 1
    boundary = rpb * (blocks // 2)  # the clustered top straddles this block-range boundary
    cols = [oc.ascending(nx), oc.descending(nx), oc.desc_then_asc(nx, 3 * k), oc.sawtooth(nx, rpb),
            oc.clustered_top(nx, boundary - 64, 128)]
    ranks = np.stack(cols, axis=1)
    x = oc.encode(ranks, ORD_D)
    q = oc.queries(list(ORD_PAIRS), ORD_D)
    rs, ri = oc.closed_form_topk(ranks, list(ORD_PAIRS), k)
    return x, q, rs, ri


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", [1, 100, 128])
@pytest.mark.parametrize("nx", ORD_NX)
def test_ordered_corpora(K, nx, k, dtype):
    """ascending (every row passes a running threshold: the order that
    overflowed v3 and v4), descending, desc_then_asc(3k), sawtooth(rows per
    block), a clustered top across a block boundary; exact integer scores in
    all three dtypes, closed-form expectation."""
    x, q, rs, ri = _ordered(nx, k)
    got = K.flatip_topk_online(_dev(q, dtype), _dev(x, dtype), k)
    _assert_equal(got, rs, ri, f"nx={nx} k={k} {dtype}")


# ---- 3. ties ---------------------------------------------------------------------
def test_identical_rows_at_the_largest_grid(K):
    """Every row equal (dyadic): every score of a query ties, every block list
    is full of them, and the finish resolves the union down to the id bits.
    The ids must be 0..127 for every query."""
    nx, _, _ = _largest_grid_nx()
    d, k = 32, 128
    x = np.full((nx, d), 0.5, np.float32)
    q = (np.arange(8 * d, dtype=np.float32).reshape(8, d) % 7 - 3.0) * 0.25
    want_s = np.repeat((q.astype(np.float64) @ x[0].astype(np.float64)).astype(np.float32)[:, None], k, axis=1)
    for dtype in DTYPES:
        got = K.flatip_topk_online(_dev(q, dtype), _dev(x, dtype), k)
        _assert_equal(got, want_s, np.broadcast_to(np.arange(k), (8, k)), f"identical rows {dtype}")


def test_duplicates_across_a_block_boundary(K):
    from rtrec_amd import kernels
    nx, d, k = 1000, 64, 10
    blocks, rpb = kernels.flatip_topk_online_plan(8, nx, d, F32, k)
    assert blocks > 1
    q, x, _, _ = _random_case(nx, d, seed=2)
    x = x.copy()
    best = (30.0 * q[0] / np.linalg.norm(q[0])).astype(np.float32)  # far above any random row's score
    for r in (rpb - 2, rpb - 1, rpb, rpb + 1, 2 * rpb - 1, 2 * rpb):  # both sides of two boundaries
        x[r] = best
    rs, ri = orc.flat_ip_search(q, x, k, nthreads=8)
    assert list(ri[0, :6]) == [rpb - 2, rpb - 1, rpb, rpb + 1, 2 * rpb - 1, 2 * rpb]  # lower id first
    _assert_equal(K.flatip_topk_online(_dev(q), _dev(x), k), rs, ri, "planted duplicates")


# ---- 4. exclusions, id_offset ------------------------------------------------------
def test_exclude_bits_and_id_offset(K):
    nx, d, k, off = 4097, 64, 50, 5_000_000
    q, x, rs0, ri0 = _random_case(nx, d)
    rng = np.random.default_rng(11)
    random_excl = [rng.choice(nx, 900, replace=False) for _ in range(8)]
    current_top = [ri0[j, :k] for j in range(8)]  # exclude exactly the current top-k
    for name, excl in (("random", random_excl), ("top-k", current_top)):
        bm_np = orc.exclusion_bitmap(8, nx, excl)
        rs, ri = orc.flat_ip_search(q, x, k, exclude_bits=bm_np, id_offset=off, nthreads=8)
        bm = K.exclusion_bitmap(8, nx, excl, "cuda")
        got = K.flatip_topk_online(_dev(q), _dev(x), k, exclude_bits=bm, id_offset=off)
        _assert_equal(got, rs, ri, f"exclude {name}")
        if name == "top-k":
            assert np.array_equal(ri, ri0[:, k:2 * k] + off)
    # fewer eligible rows than k: the tail is padding
    few = [np.arange(5, nx) for _ in range(3)]
    bm = K.exclusion_bitmap(3, nx, few, "cuda")
    rs, ri = orc.flat_ip_search(q[:3], x, k, exclude_bits=orc.exclusion_bitmap(3, nx, few), id_offset=off, nthreads=3)
    assert (ri[:, 5:] == -1).all()
    _assert_equal(K.flatip_topk_online(_dev(q[:3]), _dev(x), k, exclude_bits=bm, id_offset=off), rs, ri, "few left")


# ---- 5. dyadic goldens, empty corpus, caller buffers ---------------------------------
@pytest.mark.parametrize("name,k", [("flatip_dyadic_raw", 10), ("flatip_dyadic_raw", 100), ("flatip_dyadic_unit", 1),
                                    ("flatip_dyadic_unit", 100), ("flatip_dyadic_small", 10)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dyadic_goldens(K, golden, name, k, dtype):
    """Exactly summable inputs with planted exact ties (lower id wins): the
    golden rows, 8 / 8 / 5 queries at a time."""
    g = golden(name)
    x = torch.from_numpy(g["items"]).to(dtype).cuda()
    nq_all = min(g["queries"].shape[0], 21)
    for q0 in range(0, nq_all, 8):
        q1 = min(q0 + 8, nq_all)
        q = torch.from_numpy(g["queries"][q0:q1]).to(dtype).cuda()
        _assert_equal(K.flatip_topk_online(q, x, k), g[f"k{k}_scores"][q0:q1], g[f"k{k}_ids"][q0:q1],
                      f"{name} k={k} queries {q0}:{q1}")


def test_dyadic_golden_exclusion(K, golden):
    g = golden("flatip_dyadic_raw")
    bm = torch.from_numpy(g["exclude_bits"][:8].view(np.int32)).cuda()
    got = K.flatip_topk_online(torch.from_numpy(g["queries"][:8]).cuda(), torch.from_numpy(g["items"]).cuda(), 100,
                               exclude_bits=bm)
    _assert_equal(got, g["excl_k100_scores"][:8], g["excl_k100_ids"][:8], "golden exclusion")


def test_empty_corpus_is_all_padding(K):
    q = torch.randn(3, 128, device="cuda")
    x = torch.empty(0, 128, device="cuda")
    gs, gi = K.flatip_topk_online(q, x, 7)
    torch.cuda.synchronize()
    assert (gi.cpu().numpy() == -1).all() and (gs.cpu().numpy() == NEG).all()


def test_agrees_with_flatip_topk_and_takes_caller_buffers(K):
    from rtrec_amd import native
    q, x, rs, ri = _random_case(4097, 128)
    qd, xd = _dev(q), _dev(x)
    out = (torch.empty(8, 50, device="cuda"), torch.empty(8, 50, dtype=torch.int64, device="cuda"))
    ws = torch.empty(native.lib().rt_flatip_topk_online_workspace_bytes(8, 4097, 128, native.RT_F32, 50),
                     dtype=torch.uint8, device="cuda")
    gs, gi = K.flatip_topk_online(qd, xd, 50, out=out, workspace_buf=ws)
    assert gs is out[0] and gi is out[1]
    es, ei = K.flatip_topk(qd, xd, 50)
    torch.cuda.synchronize()
    assert torch.equal(gs, es) and torch.equal(gi, ei)
    with pytest.raises(native.RTError):
        K.flatip_topk_online(torch.randn(9, 128, device="cuda"), xd, 10)
    with pytest.raises(native.RTError):
        K.flatip_topk_online(qd, xd, 129)
