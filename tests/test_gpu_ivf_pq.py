"""rt_pq_encode and rt_ivf_pq_topk (csrc/ivf_pq.hip) against the fp64 restatement
of tests/_ivf_pq_ref.py, on hand-made lists (no training). One layout of 8 lists
(0, 1, 37, 255, 256, 257, 600, 1500 rows) serves every search: at the default
plan a chunk is one 256-row tile, so the 600-row list takes three chunks; with
the chunk floor at 8 tiles the 1500-row list, stored in ascending score order
for query 0, is one block whose 448-entry buffer compacts more than once.
Dyadic inputs (multiples of 2^-4 in [-2, 2]) make every fp32 sum exact: scores,
ids and order equal the reference's. Gaussian inputs: _ivf_pq_ref.check_topk
with tol = (dsub + M + 2) 2^-24 (|bias| + sum |q_j c_j|), the first-order bound of
a dsub-long fmaf chain per table entry and M + 1 additions, plus one for the rest."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _ivf_pq_ref as ref

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 37, 255, 256, 257, 600, 1500]
NLIST, N, ASC_LIST, MLR = len(LENGTHS), sum(LENGTHS), 7, max(LENGTHS)
SHAPES = [(32, 4), (32, 8), (128, 16), (128, 32), (128, 64)]   # 4-byte codes, 16-byte, two uint4, the LDS maximum
shapes = pytest.mark.parametrize("d,M", SHAPES, ids=[f"d{d}-M{M}" for d, M in SHAPES])
families = pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "gauss"])
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels
    yield kernels
    kernels.ivf_topk_tuning(0)


def _draw(rng, shape, dyadic):
    return (rng.integers(-32, 33, shape) / 16.0 if dyadic else rng.standard_normal(shape)).astype(np.float32)


def _bits(exclude):
    packed = np.zeros((len(exclude), (exclude.shape[1] + 31) // 32 * 32), bool)
    packed[:, :exclude.shape[1]] = exclude
    return torch.from_numpy(np.packbits(packed, axis=1, bitorder="little").view(np.int32).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _case(d, M, dyadic):
    """queries [5, d], codebooks, codes [N, M] (stored order), offsets, row_pos."""
    rng = np.random.default_rng(1000 * d + M + (7 if dyadic else 0))
    q, cb = _draw(rng, (5, d), dyadic), _draw(rng, (M, 256, d // M), dyadic)
    codes = rng.integers(0, 256, (N, M))
    if dyadic:   # half the rows draw from 4 codewords: plenty of equal scores
        few = rng.random(N) < 0.5
        codes[few] = rng.integers(0, 4, (int(few.sum()), M))
    codes = codes.astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    lo, hi = offsets[ASC_LIST], offsets[ASC_LIST + 1]
    s0 = ref.tables(q[:1], cb)[0][0, np.arange(M), codes[lo:hi].astype(np.int64)].sum(axis=1)
    codes[lo:hi] = codes[lo:hi][np.argsort(s0, kind="stable")]
    return q, cb, codes, offsets, rng.permutation(N).astype(np.int32)


def _probes(nq, nprobe, rng):
    """Query 0 probes the ascending list first; with nq = 5, query 1 probes the lists
    of 1, 0 and 37 rows first (fewer than k rows) and the last query starts with -1;
    with nprobe > 1 query 0 ends with an entry >= nlist."""
    p = np.stack([rng.permutation(NLIST) for _ in range(nq)]).astype(np.int64)
    p[0] = [ASC_LIST] + [l for l in p[0] if l != ASC_LIST]
    if nq > 1:
        p[1] = [1, 0, 2] + [l for l in p[1] if l not in (0, 1, 2)]
        p[nq - 1, 0] = -1
    p = np.ascontiguousarray(p[:, :nprobe])
    if nprobe > 1:
        p[0, nprobe - 1] = NLIST + 2
    return p


@pytest.mark.parametrize("min_tiles", [0, 8], ids=["chunk1", "chunk8"])
@families
@shapes
def test_adc_search(K, d, M, dyadic, min_tiles):
    K.ivf_topk_tuning(min_tiles)
    chunks, rows_per_chunk, _ = K.ivf_topk_plan(1, 8, MLR)
    assert (rows_per_chunk == 256 and chunks == 6) if min_tiles == 0 else (rows_per_chunk >= MLR and chunks == 1)
    q, cb, codes, offsets, row_pos = _case(d, M, dyadic)
    dev = [torch.from_numpy(a).cuda() for a in (codes, cb, offsets, row_pos)]
    rng = np.random.default_rng(5)
    for nq, nprobe, k, with_bias, with_excl in itertools.product([1, 5], [1, 3, 8], [1, 10, 128], [False, True],
                                                                 [False, True]):
        probes = _probes(nq, nprobe, rng)
        bias = _draw(rng, (nq, nprobe), dyadic) if with_bias else None
        exclude = None
        if with_excl:   # the best 5 rows of every query
            top = ref.adc_search(q[:nq], codes, cb, offsets, row_pos, probes, bias, 5)[1]
            exclude = np.zeros((nq, N), bool)
            for i in range(nq):
                exclude[i, top[i][top[i] >= 0]] = True
        got = K.ivf_pq_topk(torch.from_numpy(q[:nq]).cuda(), *dev, torch.from_numpy(probes).cuda(), MLR, k,
                            bias=None if bias is None else torch.from_numpy(bias).cuda(),
                            exclude_bits=None if exclude is None else _bits(exclude))
        torch.cuda.synchronize()
        gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
        what = f"nq={nq} nprobe={nprobe} k={k} bias={with_bias} excl={with_excl}"
        if dyadic:
            rs, ri = ref.adc_search(q[:nq], codes, cb, offsets, row_pos, probes, bias, k, exclude)
            assert np.array_equal(gi, ri), what
            assert np.array_equal(gs[ri >= 0].astype(np.float64), rs[ri >= 0]), what
            assert np.all(gs[ri < 0] == -np.finfo(np.float32).max), what
        else:
            cands = ref.adc_scores(q[:nq], codes, cb, offsets, row_pos, probes, bias, exclude)
            for i in range(nq):
                ref.check_topk(gs[i], gi[i], cands[i], k, (d // M + M + 2) * EPS)


@pytest.mark.parametrize("resid", [False, True], ids=["rows", "residual"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@families
@shapes
def test_encode(K, d, M, dyadic, dt, resid):
    """n = 300 (two row tiles, the second partial). Dyadic: the reference's codes
    exactly, rows equidistant from two codewords (a duplicated codeword) and
    rows whose assign is outside [0, nlist) included. Gaussian: the fp64
    distance of the chosen codeword is within E(chosen) + E(best) of the
    minimum, E(c) = (dsub + 3) 2^-24 sum_j (t_j^2 + 2 |r_j| t_j), t = |r - c|: the
    fp32 residual, the difference, the square and a dsub-long chain, first order."""
    n, nlist, dsub = 300, 6, d // M
    rng = np.random.default_rng(d + M)
    cb, cen = _draw(rng, (M, 256, dsub), dyadic), _draw(rng, (nlist, d), dyadic)
    cb[:, 200] = cb[:, 17]
    assign = rng.integers(0, nlist, n).astype(np.int64)
    assign[5], assign[6] = -1, nlist
    inside = ((assign >= 0) & (assign < nlist))[:, None]
    shift = np.where(inside, cen[assign % nlist], 0) if resid else np.zeros((n, d), np.float32)
    x = torch.from_numpy(_draw(rng, (n, d), dyadic)).to(dt).float().numpy()
    if dyadic:   # rows 0..19 sit on codeword 17 (= 200) of every subspace
        x[:20] = cb[:, 17].reshape(-1) + shift[:20]
    args = (torch.from_numpy(cen).cuda(), torch.from_numpy(assign).cuda()) if resid else ()
    got = K.pq_encode(torch.from_numpy(x).to(dt).cuda(), torch.from_numpy(cb).cuda(), *args)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want, dist = ref.encode(x, cb, cen if resid else None, assign if resid else None)
    if dyadic:
        assert np.array_equal(got, want) and np.all(got[:5] == 17)
        return
    r = (x.astype(np.float64) - shift).reshape(n, M, 1, dsub)
    t = np.abs(r - cb[None].astype(np.float64))
    E = (dsub + 3) * EPS * (t * t + 2 * np.abs(r) * t).sum(axis=3)
    rows, ms = np.arange(n)[:, None], np.arange(M)[None]
    g, w = got.astype(np.int64), want.astype(np.int64)
    assert np.all(dist[rows, ms, g] <= dist[rows, ms, w] + E[rows, ms, g] + E[rows, ms, w])


def test_graph_capture(K):
    """Captured in a torch.cuda.graph and replayed three times: the eager result."""
    K.ivf_topk_tuning(0)
    M, nq, k, nprobe = 16, 5, 10, 8
    q, cb, codes, offsets, row_pos = _case(128, M, True)
    probes = _probes(nq, nprobe, np.random.default_rng(2))
    bias = _draw(np.random.default_rng(3), (nq, nprobe), True)
    ops = [torch.from_numpy(a).cuda() for a in (q[:nq], codes, cb, offsets, row_pos, probes)]
    kw = dict(bias=torch.from_numpy(bias).cuda(), workspace_buf=torch.empty(
        K.native.lib().rt_ivf_pq_topk_workspace_bytes(nq, nprobe, MLR, k, M), dtype=torch.uint8, device="cuda"))
    eager = K.ivf_pq_topk(*ops, MLR, k, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(eager[1].cpu().numpy(), ref.adc_search(q[:nq], codes, cb, offsets, row_pos, probes, bias, k)[1])
    out = (torch.empty_like(eager[0]), torch.empty_like(eager[1]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        K.ivf_pq_topk(*ops, MLR, k, out=out, **kw)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
