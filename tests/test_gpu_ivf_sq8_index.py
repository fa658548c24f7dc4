"""HipIVFSQ8Index on tests/_ivf_ref.py's clustered corpus (8192 x 32), "IVF16,SQ8", nprobe 4,
cosine: searches against the fp64 restatement run on the index's OWN codes, lo, step, probes
and coarse scores (bound of test_gpu_ivf_sq8.py), add / save / load, the engine, the refusals."""
import numpy as np
import pytest
import torch

import _ivf_sq8_ref as ref
from _ivf_pq_ref import check_topk
from _ivf_ref import clustered_corpus
from test_gpu_ivf_pq_index import R  # noqa: F401  (the module fixture: rtrec_amd.serving.retrieval)

pytestmark = pytest.mark.gpu

D, NLIST, NPROBE, K10 = 32, 16, 4, 10
FACTOR = (D + 4) * 2.0 ** -24


def _config(**kw):
    return dict(dimension=D, metric="cosine", index_factory=f"IVF{NLIST},SQ8", nprobe=NPROBE, **kw)


def _build(by_residual=True, n=8192):
    from rtrec_amd.serving.retrieval import HipIVFSQ8Index
    index = HipIVFSQ8Index(_config(by_residual=by_residual))
    index.build(clustered_corpus()[0][:n], [f"item{i}" for i in range(n)])
    return index


def _check_search(index, queries, k=K10):
    """search_tensors against ref.scores over the index's own state."""
    q32 = index._prepare(queries)
    coarse, probes = index.coarse_search(q32, NPROBE)
    gs, gi = index.search_tensors(queries, k)
    torch.cuda.synchronize()
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert index.codes.dtype == torch.uint8 and tuple(index.codes.shape) == (index.current_size, D)
    state = [t.cpu().numpy() for t in (q32, index.codes, index.lo, index.step, index.list_offsets, index.row_pos, probes)]
    cands = ref.scores(*state, coarse.cpu().numpy() if index.by_residual else None)
    for i in range(len(queries)):
        check_topk(gs[i], gi[i], cands[i], k, FACTOR)
    return gs, gi


@pytest.mark.parametrize("by_residual", [True, False], ids=["residual", "rows"])
def test_search_and_reconstruction(R, by_residual):
    """vectors() lies within step_j (0.5 + 2^-10) of the prepared rows: the range is the exact
    minimum and maximum of the build rows, so no value clamps."""
    index = _build(by_residual)
    _check_search(index, clustered_corpus()[1][:64])
    rows = index._prepare(clustered_corpus()[0]).cpu().numpy().astype(np.float64)
    step = index.step.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(index.vectors() - rows) <= step * (0.5 + 2.0 ** -10))


def test_add_save_load(R, tmp_path):
    rows, queries = clustered_corpus()
    index = _build(True, 7000)
    quant = [t.clone() for t in (index.lo, index.step, index.inv_step)]
    index.add(rows[7000:], [f"item{i}" for i in range(7000, len(rows))])
    assert index.current_size == len(rows)
    assert all(torch.equal(a, b) for a, b in zip(quant, (index.lo, index.step, index.inv_step)))
    gs, gi = _check_search(index, queries[:32])
    assert (gi >= 7000).any()
    index.save(str(tmp_path / "sq8"))
    loaded = R.HipIVFSQ8Index(_config())
    loaded.load(str(tmp_path / "sq8"))
    ls, li = _check_search(loaded, queries[:32])
    assert np.array_equal(gi, li) and np.array_equal(gs, ls)
    assert loaded.search(queries[:2], 5)[0] == index.search(queries[:2], 5)[0]


def test_engine_and_refusals(R):
    rows, queries = clustered_corpus()
    engine = R.RetrievalEngine({"index_type": "hip_ivf_sq8", "embedding_dim": D, "top_k": K10,
                                "hip_ivf_sq8": _config()})
    assert isinstance(engine.index, R.HipIVFSQ8Index) and engine.index.by_residual
    engine.build_index(rows, [f"item{i}" for i in range(len(rows))])
    ids, scores, _ = engine.retrieve(queries[:4])
    assert all(len(r) == K10 and len(set(r)) == K10 for r in ids)
    assert all(s == sorted(s, reverse=True) for s in scores)
    for bad in ({"index_factory": "IVF16,SQ4"}, {"index_factory": "IVF16,Flat"}, {"dimension": 40}):
        with pytest.raises(ValueError, match="SQ8|d % 16"):
            R.HipIVFSQ8Index(_config() | bad)
    with pytest.raises(ValueError, match="HipIVFFlatIndex"):
        engine.index.search(queries[:1], 5, mmr_lambda=0.5)
    for key in ("batch_min_queries", "online_max_batch"):
        with pytest.raises(ValueError, match="HipIVFSQ8Index.*HipIVFFlatIndex"):
            R.HipIVFSQ8Index(_config(**{key: 8}))
    with pytest.raises(NotImplementedError, match="HipMutableIVFFlatIndex"):
        engine.index.remove(["item0"])
