"""rt_refine_topk through kernels.refine_topk against tests/_refine_ref.py (fp64): 300 rows (10 and
11 equal), every kind, d of one partial / whole k-steps, n_cand around the wave boundary."""
import numpy as np
import pytest
import torch

import _refine_ref as ref

pytestmark = pytest.mark.gpu

N_ROWS = 300
KIND_D = [(kind, d) for kind in ("f32", "f16", "bf16", "sq8")
          for d in (16, 128, 256, 72 if kind == "f32" else 136) if not (kind == "sq8" and d == 136)]
CAND_K = [(n, k) for n in (1, 63, 64, 65, 128) for k in sorted({1, min(10, n), n})]
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def kernels():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels
    return kernels


def _candidates(rng, nq, n_cand):
    """Query 0: -1 in the middle, id == n_rows, a repeat, both equal rows; query 3: all absent."""
    ids = rng.integers(0, N_ROWS, (nq, n_cand))
    if n_cand >= 63:
        ids[0, [0, 1, 2, n_cand // 2, -1]] = [10, N_ROWS, ids[0, 3], -1, 11]
    if nq > 3:
        ids[3] = np.where(np.arange(n_cand) % 2 == 0, -1, N_ROWS + np.arange(n_cand))
    return ids


def _inputs(kind, d, nq, n_cand, dyadic, seed=0):
    """(queries fp32, cand_ids, store tensor, lo, step, fp64 rows of the store)."""
    rng = np.random.default_rng(seed)
    ids = _candidates(rng, nq, n_cand)
    draw = (lambda *s: rng.integers(-32, 33, s) / 16.0) if dyadic else (lambda *s: rng.standard_normal(s))
    q = draw(nq, d).astype(np.float32)
    lo = step = None
    if kind == "sq8":
        store = torch.from_numpy(rng.integers(0, 256, (N_ROWS, d)).astype(np.uint8))
        lo = (rng.integers(-2, 0, d).astype(np.float32) if dyadic else -3 - rng.random(d).astype(np.float32))
        step = np.full(d, 2.0 ** -4, np.float32) if dyadic else ((6 + rng.random(d)) / 255).astype(np.float32)
    else:
        store = torch.from_numpy(draw(N_ROWS, d).astype(np.float32)).to(DTYPES[kind])
    store[11] = store[10]
    rows = ref.decode(store.float().numpy(), lo, step)
    return q, ids, store, lo, step, rows


def _run(kernels, q, ids, store, lo, step, k):
    dev = lambda a: None if a is None else torch.as_tensor(a).cuda()   # noqa: E731
    s, i = kernels.refine_topk(dev(q), dev(ids), dev(store), k, lo=dev(lo), step=dev(step))
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("n_cand,k", CAND_K)
@pytest.mark.parametrize("kind,d", KIND_D)
@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "gaussian"])
def test_against_fp64(kernels, dyadic, kind, d, n_cand, k, nq):
    """Dyadic (multiples of 2^-4 in [-2, 2]; SQ8: lo in {-2, -1}, step 2^-4): every fp32 sum is exact, so
    positions, order and scores are the fp64 list's. Gaussian: tol = (d + 2) 2^-24 sum |q_j x_j|, the
    first-order bound of the sequential chain."""
    q, ids, store, lo, step, rows = _inputs(kind, d, nq, n_cand, dyadic)
    gs, gi = _run(kernels, q, ids, store, lo, step, k)
    ws, wi, cands = ref.refine(q, ids, rows, k)
    if dyadic:
        assert np.array_equal(gi, wi)
        assert np.array_equal(gs.astype(np.float64), np.where(wi >= 0, ws, -np.finfo(np.float32).max))
    for i in range(nq):
        ref.check(gs[i], gi[i], cands[i], k, (d + 2) * 2.0 ** -24)


def test_f32_scores_are_flatip_topk_bits(kernels):
    """An fp32 store gives rt_flatip_topk's score of the same (query, row), bit for bit."""
    q, _, store, _, _, _ = _inputs("f32", 72, 5, 128, dyadic=False)
    fs, fi = kernels.flatip_topk(torch.from_numpy(q).cuda(), store.cuda(), 128)
    gs, gi = kernels.refine_topk(torch.from_numpy(q).cuda(), fi.flip(1).contiguous(), store.cuda(), 128)
    torch.cuda.synchronize()
    assert torch.equal(gi, fi) and torch.equal(gs.view(torch.int32), fs.view(torch.int32))
