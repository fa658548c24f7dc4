"""The ``sq8_batch_min_queries`` key of HipIVFSQ8Index on tests/_ivf_ref.py's clustered corpus
(8192 x 32), "IVF16,SQ8", nprobe 4, cosine: an index with the key answers exactly as one
without it (ids and score bits), calls of that many queries take kernels.ivf_sq8_topk_batch,
and the key travels through save / load, RetrievalEngine and evaluation.build_eval_index."""
import numpy as np
import pytest
import torch

from _ivf_ref import clustered_corpus
from test_gpu_ivf_pq_index import R  # noqa: F401  (the module fixture: rtrec_amd.serving.retrieval)
from test_gpu_ivf_sq8_index import D, _config

pytestmark = pytest.mark.gpu
CATS = ["a", "b", "c"]
N = 8192
IDS = [f"item{i}" for i in range(N)]


@pytest.fixture(scope="module")
def pair(R):
    """(index without the key, index with sq8_batch_min_queries = 16) over the same rows."""
    cats = [[CATS[p % 3]] if p % 7 else [] for p in range(N)]
    out = []
    for extra in ({}, {"sq8_batch_min_queries": 16}):
        index = R.HipIVFSQ8Index(_config(categories=CATS, **extra))
        index.build(clustered_corpus()[0], IDS, item_categories=cats)
        out.append(index)
    assert torch.equal(out[0].codes, out[1].codes) and torch.equal(out[0].row_pos, out[1].row_pos)
    assert out[0].sq8_batch_min_queries is None and out[1].sq8_batch_min_queries == 16
    return out


def _same(a, b):
    torch.cuda.synchronize()
    assert np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert np.array_equal(a[0].cpu().numpy().view(np.uint32), b[0].cpu().numpy().view(np.uint32))


def _spy(monkeypatch, kernels):
    calls = []
    real = kernels.ivf_sq8_topk_batch
    monkeypatch.setattr(kernels, "ivf_sq8_topk_batch", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    return calls


def test_search_equal_and_dispatch(R, pair, monkeypatch):
    plain, keyed = pair
    queries = clustered_corpus()[1]
    calls = _spy(monkeypatch, R.kernels)
    for k in (10, 100):
        _same(keyed.search_tensors(queries[:64], k), plain.search_tensors(queries[:64], k))
    assert calls == [64, 64]
    keyed.search_tensors(queries[:15], 10)
    assert calls == [64, 64]
    _same(keyed.search_tensors(queries[:16], 10), plain.search_tensors(queries[:16], 10))
    assert calls == [64, 64, 16]
    q = queries[:64]
    own = [ids[:3] for ids in plain.search(q, 10)[0]]   # per query: its own top three
    for kw in (dict(exclude_ids=own), dict(exclude_ids=IDS[:300]), dict(filter_categories=["a", "b"]),
               dict(exclude_categories=["c"], exclude_ids=own)):
        got = keyed.search(q, 10, **kw)
        assert got == plain.search(q, 10, **kw), kw
        assert len(calls) == 4 and calls.pop() == 64, kw
    assert all(not set(g) & set(e) for g, e in zip(keyed.search(q, 10, exclude_ids=own)[0], own))


def test_save_load_engine_and_refusals(R, pair, tmp_path, monkeypatch):
    plain, keyed = pair
    rows, queries = clustered_corpus()
    keyed.save(str(tmp_path / "sq8"))
    loaded = R.HipIVFSQ8Index(_config())
    loaded.load(str(tmp_path / "sq8"))
    assert loaded.sq8_batch_min_queries == 16
    calls = _spy(monkeypatch, R.kernels)
    _same(loaded.search_tensors(queries[:32], 10), plain.search_tensors(queries[:32], 10))
    engine = R.RetrievalEngine({"index_type": "hip_ivf_sq8", "embedding_dim": D,
                                "hip_ivf_sq8": _config(sq8_batch_min_queries=16)})
    assert engine.index.sq8_batch_min_queries == 16
    engine.build_index(rows, IDS)
    got = engine.retrieve(queries[:32], k=10, use_cache=False)
    assert calls == [32, 32] and got[0] == plain.search(queries[:32], 10)[0]
    small = R.HipIVFSQ8Index(_config(sq8_batch_min_queries=1))   # the Flat fallback ignores the key
    small.build(rows[:500], IDS[:500])
    assert len(small.search(queries[:4], 5)[0][0]) == 5 and calls == [32, 32]
    with pytest.raises(ValueError, match="sq8_batch_min_queries"):
        R.HipIVFSQ8Index(_config(batch_min_queries=8))
    with pytest.raises(ValueError, match="sq8_batch_min_queries"):
        R.HipIVFSQ8Index(_config(sq8_batch_min_queries=0))
    with pytest.raises(ValueError, match="HipIVFPQIndex.*HipIVFSQ8Index"):
        R.HipIVFPQIndex(dict(dimension=D, index_factory="IVF16,PQ8", sq8_batch_min_queries=8))


@pytest.mark.parametrize("index_type,factory", [("hip_ivf_sq8", "IVF16,SQ8"), ("hip_ivf_pq", "IVF16,PQ8")])
def test_build_eval_index(R, index_type, factory, monkeypatch):
    """The evaluation's index builds for the code-index classes and answers as the per-query index
    of the same configuration does; for SQ8 through the list-major scan."""
    from rtrec_amd.evaluation.offline import build_eval_index
    rows, queries = clustered_corpus()
    item_emb = torch.from_numpy(rows).cuda()
    cfg = {"index_type": index_type, "index_factory": factory, "nprobe": 4}
    calls = _spy(monkeypatch, R.kernels)
    index = build_eval_index(item_emb, cfg)
    assert getattr(index, "batch_min_queries", None) is None
    assert index.sq8_batch_min_queries == (1 if index_type == "hip_ivf_sq8" else None)
    got = index.search_tensors(queries[:48], 10)
    assert calls == ([48] if index_type == "hip_ivf_sq8" else [])
    per_query = R._INDEX_TYPES[index_type](dict(dimension=D, metric="inner_product", index_factory=factory, nprobe=4))
    per_query.build(item_emb, [str(i) for i in range(N)])
    _same(got, per_query.search_tensors(queries[:48], 10))
