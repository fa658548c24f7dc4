"""HipIVFPQIndex on the clustered corpus of tests/_ivf_ref.py (8192 x 32), "IVF16,PQ8",
cosine: searches against the fp64 ADC restatement run on the index's OWN downloaded
codes, codebooks, probes and coarse scores (conditions and bound of test_gpu_ivf_pq.py),
Lloyd's monotonicity, save / load / add, the engine, the documented refusals."""
import functools

import numpy as np
import pytest
import torch

import _ivf_pq_ref as ref
from _ivf_ref import clustered_corpus

pytestmark = pytest.mark.gpu

D, M, NLIST, NPROBE, K10 = 32, 8, 16, 4, 10
FACTOR = (D // M + M + 2) * 2.0 ** -24


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd.serving import retrieval
    return retrieval


def _config(**kw):
    return dict(dimension=D, metric="cosine", index_factory=f"IVF{NLIST},PQ{M}", nprobe=NPROBE, **kw)


def _build(by_residual=True, pq_train_iters=25, n=8192):
    from rtrec_amd.serving.retrieval import HipIVFPQIndex
    index = HipIVFPQIndex(_config(by_residual=by_residual, pq_train_iters=pq_train_iters))
    index.build(clustered_corpus()[0][:n], [f"item{i}" for i in range(n)])
    return index


_built = functools.lru_cache(maxsize=None)(_build)   # shared, never changed


def _check_search(index, queries, k=K10):
    """search_tensors against adc_scores over the index's own state."""
    q32 = index._prepare(queries)
    coarse, probes = index.coarse_search(q32, NPROBE)
    gs, gi = index.search_tensors(queries, k)
    torch.cuda.synchronize()
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert index.codes.dtype == torch.uint8 and tuple(index.codes.shape) == (index.current_size, M)
    state = [t.cpu().numpy() for t in (q32, index.codes, index.codebooks, index.list_offsets, index.row_pos, probes)]
    cands = ref.adc_scores(*state, coarse.cpu().numpy() if index.by_residual else None)
    for i in range(len(queries)):
        ref.check_topk(gs[i], gi[i], cands[i], k, FACTOR)
    return gs, gi


def _mse(index, rows):
    """fp64 mean squared error of the reconstruction over (normalised) rows."""
    x = rows.astype(np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    codes = np.empty((index.current_size, M), np.int64)
    codes[index.row_pos.cpu().numpy()] = index.codes.cpu().numpy()
    cb = index.codebooks.cpu().numpy().astype(np.float64)
    rec = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
    if index.by_residual:
        rec += index.centroids.cpu().numpy().astype(np.float64)[index.assign.cpu().numpy()]
    return float(((x - rec) ** 2).sum(axis=1).mean()), rec


@pytest.mark.parametrize("by_residual", [True, False], ids=["residual", "rows"])
def test_search_matches_adc(R, by_residual):
    _check_search(_built(by_residual), clustered_corpus()[1][:64])


def test_training_lowers_reconstruction_error(R):
    rows, _ = clustered_corpus()
    before, _ = _mse(_built(True, 0), rows)
    after, rec = _mse(_built(True, 25), rows)
    assert after <= before, (after, before)
    assert np.allclose(_built(True, 25).vectors(), rec, atol=1e-6)   # vectors() is the reconstruction


def test_add_save_load(R, tmp_path):
    rows, queries = clustered_corpus()
    index = _build(True, 25, 7000)
    codebooks = index.codebooks.clone()
    index.add(rows[7000:], [f"item{i}" for i in range(7000, len(rows))])
    assert index.current_size == len(rows) and torch.equal(index.codebooks, codebooks)
    gs, gi = _check_search(index, queries[:32])
    assert (gi >= 7000).any()
    index.save(str(tmp_path / "pq"))
    loaded = R.HipIVFPQIndex(_config())
    loaded.load(str(tmp_path / "pq"))
    ls, li = _check_search(loaded, queries[:32])
    assert np.array_equal(gi, li) and np.array_equal(gs, ls)
    assert loaded.search(queries[:2], 5)[0] == index.search(queries[:2], 5)[0]


def test_engine_and_refusals(R):
    rows, queries = clustered_corpus()
    engine = R.RetrievalEngine({"index_type": "hip_ivf_pq", "embedding_dim": D, "top_k": K10,
                                "hip_ivf_pq": _config(pq_train_iters=2)})
    assert isinstance(engine.index, R.HipIVFPQIndex)
    engine.build_index(rows, [f"item{i}" for i in range(len(rows))])
    ids, scores, _ = engine.retrieve(queries[:4])
    assert all(len(r) == K10 and len(set(r)) == K10 for r in ids)
    assert all(s == sorted(s, reverse=True) for s in scores)
    with pytest.raises(ValueError, match="8 bits per code"):
        R.HipIVFPQIndex(_config() | {"index_factory": "IVF16,PQ8x4"})
    assert R.HipIVFPQIndex(_config() | {"index_factory": "IVF16,PQ8x8"}).pq_m == 8
    with pytest.raises(ValueError, match="HipIVFFlatIndex"):
        engine.index.search(queries[:1], 5, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="HipIVFFlatIndex"):
        R.HipIVFPQIndex(_config(batch_min_queries=64))
    with pytest.raises(NotImplementedError, match="HipMutableIVFFlatIndex"):
        engine.index.remove(["item0"])
