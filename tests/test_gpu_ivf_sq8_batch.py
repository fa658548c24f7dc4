"""rt_ivf_sq8_topk_batch (csrc/ivf_sq8_batch.hip), the list-major SQ8 scan, against
tests/_ivf_sq8_ref.py on the hand-made lists of test_gpu_ivf_pq.py and the cases of
test_gpu_ivf_sq8.py (d = 16, 128, 144, 256: one unit, exactly one step, a step plus a partial
one, two steps). 65 more queries of the same family follow the case's five: with 70 queries
that all name the 1,500-row list first, that list has two full query tiles and one of 6, in two
chunks. Dyadic: ids, order and scores equal the fp64 reference. Gaussian: check_topk with the
bound (d + 4) 2^-24 of test_gpu_ivf_sq8.py. Both: ids and score bits equal kernels.ivf_sq8_topk."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _ivf_sq8_ref as ref
from _ivf_pq_ref import check_topk
from test_gpu_ivf_pq import ASC_LIST, EPS, MLR, N, NLIST, K, _bits, _probes, families  # noqa: F401  (K: fixture)
from test_gpu_ivf_sq8 import _bias, _case, dims

pytestmark = pytest.mark.gpu
NQ = 70


@functools.lru_cache(maxsize=None)
def _queries(d, dyadic):
    rng = np.random.default_rng(9 * d + dyadic)
    more = rng.integers(-8, 9, (NQ - 5, d)) / 8.0 if dyadic else rng.standard_normal((NQ - 5, d))
    return np.concatenate([_case(d, dyadic)[0], more.astype(np.float32)])


def _probe_table(nq, nprobe, rng):
    """nq <= 5: test_gpu_ivf_pq's table (-1, an id >= nlist, the lists shorter than k). nq = 70:
    every query names the ascending 1,500-row list first; with nprobe = 8 query 0 ends with an id
    >= nlist and the last query has a -1."""
    if nq <= 5:
        return _probes(nq, nprobe, rng)
    p = np.stack([[ASC_LIST] + [l for l in rng.permutation(NLIST) if l != ASC_LIST] for _ in range(nq)])
    p = np.ascontiguousarray(p[:, :nprobe]).astype(np.int64)
    if nprobe > 1:
        p[0, nprobe - 1], p[nq - 1, 3] = NLIST + 2, -1
    return p


@families
@dims
@pytest.mark.parametrize("nq", [1, 5, NQ])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_search(K, d, dyadic, nq, k):
    assert K.ivf_topk_batch_plan(NQ, 8, NLIST, MLR, 128)[1:3] == (1024, 2)   # two chunks of the long list
    _, lo, step, codes, offsets, row_pos = _case(d, dyadic)
    q = _queries(d, dyadic)
    dev = [torch.from_numpy(a).cuda() for a in (codes, lo, step, offsets, row_pos)]
    rng = np.random.default_rng(5)
    for nprobe, with_bias, with_excl in itertools.product([1, 8], [False, True], [False, True]):
        probes = _probe_table(nq, nprobe, rng)
        bias = _bias(rng, (nq, nprobe), dyadic) if with_bias else None
        state = (q[:nq], codes, lo, step, offsets, row_pos, probes, bias)
        exclude = None
        if with_excl:   # the best 5 rows of every query
            top = ref.search(*state, 5)[1]
            exclude = np.zeros((nq, N), bool)
            for i in range(nq):
                exclude[i, top[i][top[i] >= 0]] = True
        args = (torch.from_numpy(q[:nq]).cuda(), *dev, torch.from_numpy(probes).cuda(), MLR, k)
        kw = dict(bias=None if bias is None else torch.from_numpy(bias).cuda(),
                  exclude_bits=None if exclude is None else _bits(exclude))
        got = K.ivf_sq8_topk_batch(*args, **kw)
        per_query = K.ivf_sq8_topk(*args, **kw)
        torch.cuda.synchronize()
        gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
        what = f"nprobe={nprobe} bias={with_bias} excl={with_excl}"
        if dyadic:
            rs, ri = ref.search(*state, k, exclude)
            assert np.array_equal(gi, ri), what
            assert np.array_equal(gs[ri >= 0].astype(np.float64), rs[ri >= 0]), what
            assert np.all(gs[ri < 0] == -np.finfo(np.float32).max), what
        else:
            cands = ref.scores(*state, exclude)
            for i in range(nq):
                try:
                    check_topk(gs[i], gi[i], cands[i], k, (d + 4) * EPS)
                except AssertionError as e:   # name the combination and the query
                    raise AssertionError(f"{what} query {i}: {e}") from e
        assert np.array_equal(gi, per_query[1].cpu().numpy()), what
        assert np.array_equal(gs.view(np.uint32), per_query[0].cpu().numpy().view(np.uint32)), what


def test_graph_capture(K):
    """Captured once; probes, queries and bias are then overwritten in place, three times: every
    replay equals the eager result on the new inputs (and the reference's ids)."""
    d, nq, k, nprobe = 144, NQ, 10, 8
    _, lo, step, codes, offsets, row_pos = _case(d, True)
    q = _queries(d, True)
    rng = np.random.default_rng(2)
    fixed = [torch.from_numpy(a).cuda() for a in (codes, lo, step, offsets, row_pos)]
    qd, pd = torch.from_numpy(q).cuda(), torch.from_numpy(_probe_table(nq, nprobe, rng)).cuda()
    bd = torch.from_numpy(_bias(rng, (nq, nprobe), True)).cuda()
    ws = torch.empty(K.native.lib().rt_ivf_sq8_topk_batch_workspace_bytes(nq, nprobe, NLIST, MLR, k, d),
                     dtype=torch.uint8, device="cuda")
    out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"),
           torch.empty((nq, k), dtype=torch.int64, device="cuda"))
    K.ivf_sq8_topk_batch(qd, *fixed, pd, MLR, k, bias=bd, workspace_buf=ws)   # warm-up outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        K.ivf_sq8_topk_batch(qd, *fixed, pd, MLR, k, bias=bd, out=out, workspace_buf=ws)
    for _ in range(3):
        q_new = q[rng.permutation(nq)]
        p_new = _probes(5, nprobe, rng)[rng.integers(0, 5, nq)]   # another grouping: no list named by all
        b_new = _bias(rng, (nq, nprobe), True)
        qd.copy_(torch.from_numpy(q_new))
        pd.copy_(torch.from_numpy(p_new))
        bd.copy_(torch.from_numpy(b_new))
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = K.ivf_sq8_topk_batch(qd, *fixed, pd, MLR, k, bias=bd)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        assert np.array_equal(out[1].cpu().numpy(), ref.search(q_new, codes, lo, step, offsets, row_pos, p_new, b_new, k)[1])
