"""rt_sq8_encode and rt_ivf_sq8_topk (csrc/ivf_sq8.hip) against tests/_ivf_sq8_ref.py on the
hand-made lists, probes and chunk floors of test_gpu_ivf_pq.py. d = 16, 128, 144, 256: one unit,
exactly one 8-unit step, a step plus a partial one, two steps. Dyadic inputs (q multiples of 2^-3
in [-1, 1], step in {2^-6, 2^-5, 2^-4}, lo and bias multiples of 2^-4) make every fp32 sum exact
(checked on the CPU for d = 256 in _case): ids, order and scores equal the reference's. Gaussian:
check_topk with tol = (d + 4) 2^-24 magnitude, first order: one rounding for qs, a d-long chain
for b0, one add, a d-long chain."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _ivf_sq8_ref as ref
from _ivf_pq_ref import check_topk
from test_gpu_ivf_pq import ASC_LIST, EPS, LENGTHS, MLR, N, K, _bits, _probes, families  # noqa: F401  (its lists, fixture)

pytestmark = pytest.mark.gpu
dims = pytest.mark.parametrize("d", [16, 128, 144, 256])


def _bias(rng, shape, dyadic):
    return (rng.integers(-32, 33, shape) / 16.0 if dyadic else rng.standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(d, dyadic):
    """queries [5, d], lo, step, codes [N, d] (stored order), offsets, row_pos."""
    rng = np.random.default_rng(100 * d + (7 if dyadic else 0))
    codes = rng.integers(0, 256, (N, d))
    if dyadic:   # half the rows draw from 4 code values: plenty of equal scores
        q, lo = rng.integers(-8, 9, (5, d)) / 8.0, rng.integers(-32, 33, d) / 16.0
        step = 2.0 ** rng.integers(-6, -3, d)
        few = rng.random(N) < 0.5
        codes[few] = rng.integers(0, 4, (int(few.sum()), d))
    else:
        q, lo, step = rng.standard_normal((5, d)), rng.standard_normal(d), rng.random(d) / 64 + 2.0 ** -8
    q, lo, step, codes = q.astype(np.float32), lo.astype(np.float32), step.astype(np.float32), codes.astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    a, b = offsets[ASC_LIST], offsets[ASC_LIST + 1]
    s0 = codes[a:b].astype(np.float64) @ (q[0].astype(np.float64) * step)
    codes[a:b] = codes[a:b][np.argsort(s0, kind="stable")]
    if dyadic and d == 256:   # the contract's chain in fp32 rounds nowhere: bias, d terms of b0, d terms of codes
        q64, mid = q.astype(np.float64), lo + 0.5 * step.astype(np.float64)
        b0 = np.cumsum(q64 * mid, axis=1)
        chain = np.cumsum((q64 * step)[:, None] * codes[None], axis=2)
        for part in [q64 * step, b0] + [b0[:, -1:, None] + bias + chain for bias in (-2.0, 0.0, 2.0)]:
            assert np.array_equal(part.astype(np.float32), part)
    return q, lo, step, codes, offsets, rng.permutation(N).astype(np.int32)


@pytest.mark.parametrize("min_tiles", [0, 8], ids=["chunk1", "chunk8"])
@families
@dims
def test_search(K, d, dyadic, min_tiles):
    K.ivf_topk_tuning(min_tiles)
    chunks, rows_per_chunk, _ = K.ivf_topk_plan(1, 8, MLR)
    assert (rows_per_chunk == 256 and chunks == 6) if min_tiles == 0 else (rows_per_chunk >= MLR and chunks == 1)
    q, lo, step, codes, offsets, row_pos = _case(d, dyadic)
    dev = [torch.from_numpy(a).cuda() for a in (codes, lo, step, offsets, row_pos)]
    rng = np.random.default_rng(5)
    for nq, nprobe, k, with_bias, with_excl in itertools.product([1, 5], [1, 3, 8], [1, 10, 128], [False, True],
                                                                 [False, True]):
        probes = _probes(nq, nprobe, rng)
        bias = _bias(rng, (nq, nprobe), dyadic) if with_bias else None
        state = (q[:nq], codes, lo, step, offsets, row_pos, probes, bias)
        exclude = None
        if with_excl:   # the best 5 rows of every query
            top = ref.search(*state, 5)[1]
            exclude = np.zeros((nq, N), bool)
            for i in range(nq):
                exclude[i, top[i][top[i] >= 0]] = True
        got = K.ivf_sq8_topk(torch.from_numpy(q[:nq]).cuda(), *dev, torch.from_numpy(probes).cuda(), MLR, k,
                             bias=None if bias is None else torch.from_numpy(bias).cuda(),
                             exclude_bits=None if exclude is None else _bits(exclude))
        torch.cuda.synchronize()
        gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
        what = f"nq={nq} nprobe={nprobe} k={k} bias={with_bias} excl={with_excl}"
        if dyadic:
            rs, ri = ref.search(*state, k, exclude)
            assert np.array_equal(gi, ri), what
            assert np.array_equal(gs[ri >= 0].astype(np.float64), rs[ri >= 0]), what
            assert np.all(gs[ri < 0] == -np.finfo(np.float32).max), what
        else:
            cands = ref.scores(*state, exclude)
            for i in range(nq):
                check_topk(gs[i], gi[i], cands[i], k, (d + 4) * EPS)


@pytest.mark.parametrize("resid", [False, True], ids=["rows", "residual"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@families
@dims
def test_encode(K, d, dyadic, dt, resid):
    """Dyadic (rows multiples of 2^-6 in [-4, 4), exact in bf16; inv_step in {16, 32, 64}: values on
    bin edges; lo in [-1, 0]: values below lo and above hi; inv_step[3] = 0): the reference's codes.
    Gaussian: a code differs from the fp64 code by at most 1, and only where the fp64 t is within
    2^-14 of an integer (3 x 255 x 2^-24: the residual, the subtraction of lo, the product)."""
    n, nlist = 300, 6
    rng = np.random.default_rng(d + 1)
    assign = rng.integers(0, nlist, n).astype(np.int64)
    assign[5], assign[6] = -1, nlist
    if dyadic:
        x, cen = rng.integers(-256, 256, (n, d)) / 64.0, rng.integers(-32, 33, (nlist, d)) / 16.0
        lo, inv = rng.integers(-16, 1, d) / 16.0, 2.0 ** rng.integers(4, 7, d)
        inv[3] = 0.0
    else:
        x, cen = rng.standard_normal((n, d)), rng.standard_normal((nlist, d)) / 4
    x = torch.from_numpy(x.astype(np.float32)).to(dt).float().numpy()
    cen = cen.astype(np.float32)
    if not dyadic:
        r = x[2:] - cen[assign[2:] % nlist] if resid else x[2:]
        lo = r.min(axis=0)
        inv = np.float32(255.0) / (r.max(axis=0) - lo)
        x[0], x[1] = 8.0, -8.0
    lo, inv = lo.astype(np.float32), inv.astype(np.float32)
    args = (torch.from_numpy(cen).cuda(), torch.from_numpy(assign).cuda()) if resid else ()
    got = K.sq8_encode(torch.from_numpy(x).to(dt).cuda(), torch.from_numpy(lo).cuda(), torch.from_numpy(inv).cuda(),
                       *args)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want, t = ref.encode(x, lo, inv, cen if resid else None, assign if resid else None)
    if dyadic:
        assert np.array_equal(got, want) and np.all(got[:, 3] == 0) and (want == 255).any() and (t < 0).any()
        return
    diff = got.astype(np.int64) != want
    assert np.all(np.abs(got.astype(np.int64) - want)[diff] == 1)
    assert np.all(np.abs(t - np.rint(t))[diff] <= 2.0 ** -14)
    assert np.all(got[0] == 255) and np.all(got[1] == 0)


def test_graph_capture(K):
    """Captured in a torch.cuda.graph and replayed three times: the eager result."""
    K.ivf_topk_tuning(0)
    d, nq, k, nprobe = 144, 5, 10, 8
    q, lo, step, codes, offsets, row_pos = _case(d, True)
    probes = _probes(nq, nprobe, np.random.default_rng(2))
    bias = _bias(np.random.default_rng(3), (nq, nprobe), True)
    ops = [torch.from_numpy(a).cuda() for a in (q[:nq], codes, lo, step, offsets, row_pos, probes)]
    kw = dict(bias=torch.from_numpy(bias).cuda(), workspace_buf=torch.empty(
        K.native.lib().rt_ivf_sq8_topk_workspace_bytes(nq, nprobe, MLR, k, d), dtype=torch.uint8, device="cuda"))
    eager = K.ivf_sq8_topk(*ops, MLR, k, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(eager[1].cpu().numpy(), ref.search(q[:nq], codes, lo, step, offsets, row_pos, probes, bias, k)[1])
    out = (torch.empty_like(eager[0]), torch.empty_like(eager[1]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        K.ivf_sq8_topk(*ops, MLR, k, out=out, **kw)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
