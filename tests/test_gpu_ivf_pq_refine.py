"""HipIVFPQIndex with a refine store on the corpus of tests/_ivf_ref.py (8192 x 32), cosine, k = 10,
nprobe 4: the refined search is the fp64 re-rank (tests/_refine_ref.py) of the unrefined candidates."""
import functools

import numpy as np
import pytest
import torch

import _refine_ref as ref
from _ivf_ref import clustered_corpus, recall_at_k

pytestmark = pytest.mark.gpu

D, K = 32, 10
FACTOR = (D + 2) * 2.0 ** -24
PLAIN, RFLAT, RSQ8 = "IVF16,PQ8", "IVF16,PQ8,RFlat", "IVF16,PQ8,Refine(SQ8)"


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd.serving import retrieval
    return retrieval


def _config(factory, **kw):
    return dict(dimension=D, metric="cosine", index_factory=factory, nprobe=4, **kw)


def _build(factory, **kw):
    from rtrec_amd.serving.retrieval import HipIVFPQIndex
    index = HipIVFPQIndex(_config(factory, **kw))
    index.build(clustered_corpus()[0], [f"item{i}" for i in range(8192)])
    return index


_built = functools.lru_cache(maxsize=None)(_build)   # shared, never changed


def _host(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("factory", [RFLAT, RSQ8])
def test_refined_search_is_the_rerank_of_the_unrefined_candidates(R, factory):
    """The candidates come from an index built with the same seed and refine off, k = 100."""
    from rtrec_amd import kernels
    index, queries, sq8 = _built(factory), clustered_corpus()[1][:64], factory == RSQ8
    cand = _built(PLAIN).search_tensors(queries, 100)[1]
    gs, gi = index.search_tensors(queries, K)
    q32 = index._prepare(queries)
    ks, ki = kernels.refine_topk(q32, cand, index.refine_store, K, lo=index.refine_lo, step=index.refine_step)
    assert torch.equal(gi, ki) and torch.equal(gs.view(torch.int32), ks.view(torch.int32))
    assert index.refine_store.dtype == (torch.uint8 if sq8 else torch.float32)
    assert tuple(index.refine_store.shape) == (8192, D)
    gs, gi, q, cand, store = _host(gs, gi, q32, cand, index.refine_store)
    rows = ref.decode(store, *(_host(index.refine_lo, index.refine_step) if sq8 else ()))
    ws, wi, cands = ref.refine(q, cand, rows, K)
    for i in range(len(q)):
        ref.check(gs[i], gi[i], cands[i], K, FACTOR)
    assert sq8 or np.array_equal(gi, wi)   # exact rows: the fp64 list itself


@pytest.mark.parametrize("first", [0, 128])
def test_recall_is_not_below_the_unrefined_index(R, first):
    rows, queries = clustered_corpus()
    queries = queries[first:first + 128]
    flat = R.HipFlatIPIndex(dict(dimension=D, metric="cosine"))
    flat.build(rows, [f"item{i}" for i in range(len(rows))])
    es, ei = _host(*flat.search_tensors(queries, K + 1))
    assert np.all(es[:, K - 1] > es[:, K]), "a tie at rank 10 in the exact lists"
    plain, refined = (recall_at_k(_host(_built(f).search_tensors(queries, K)[1])[0], ei[:, :K]) for f in (PLAIN, RFLAT))
    print(f"recall@10 queries[{first}:{first + 128}]: unrefined {plain:.4f}, RFlat {refined:.4f}")
    assert refined >= plain


def test_factory_parsing(R):
    assert [R.HipIVFPQIndex(_config(f)).refine for f in (PLAIN, RFLAT, RSQ8)] == [None, "flat", "sq8"]
    assert R._parse_ivf_pq_factory("IVF16,PQ8x8") == (16, 8, None)
    assert R.HipIVFPQIndex(_config(PLAIN, refine="sq8", refine_k_factor=4)).refine_k_factor == 4
    with pytest.raises(ValueError, match=r"RFlat.*Refine\(SQ8\)"):
        R.HipIVFPQIndex(_config("IVF16,PQ8,Refine(PQ4)"))
    with pytest.raises(ValueError, match="refine_k_factor"):
        R.HipIVFPQIndex(_config(RFLAT, refine_k_factor=0))


def test_add_save_load(R, tmp_path):
    queries = clustered_corpus()[1]
    index = _build(RFLAT, pq_train_iters=2)
    new = np.random.default_rng(1).standard_normal((5, D)).astype(np.float32)
    new /= np.linalg.norm(new, axis=1, keepdims=True)
    index.add(new, [f"new{i}" for i in range(5)])
    assert tuple(index.refine_store.shape) == (8197, D)
    gs, gi = _host(*index.search_tensors(new[2:3], K))
    exact = float(np.dot(new[2].astype(np.float64), _host(index.refine_store)[0][8194].astype(np.float64)))
    assert gi[0, 0] == 8194 and abs(float(gs[0, 0]) - exact) <= FACTOR * 1.01   # sum |q_j x_j| = 1: unit rows
    index.save(str(tmp_path / "pq"))
    loaded = R.HipIVFPQIndex(_config(PLAIN))
    loaded.load(str(tmp_path / "pq"))
    assert loaded.refine == "flat" and torch.equal(loaded.refine_store, index.refine_store)
    ws, wi = _host(*index.search_tensors(queries[:32], K))
    ls, li = _host(*loaded.search_tensors(queries[:32], K))
    assert np.array_equal(wi, li) and np.array_equal(ws.view(np.int32), ls.view(np.int32))


def test_mmr_and_exclude_ids(R):
    from rtrec_amd import kernels
    index, queries = _built(RFLAT), clustered_corpus()[1][:16]
    ids, scores = index.search(queries, 5, mmr_lambda=0.5, mmr_candidates=50)
    s, p = index.search_tensors(queries, 50)
    ms, mp = _host(*kernels.mmr_rerank(s, p, index.refine_store, 5, 0.5))
    assert ids == [[f"item{i}" for i in row] for row in mp] and np.array_equal(np.float32(scores), ms)
    with pytest.raises(ValueError, match="HipIVFFlatIndex"):
        _built(RSQ8).search(queries, 5, mmr_lambda=0.5)
    gone = [row[:3] for row in index.search(queries, K)[0]]   # an excluded item never comes back
    after = index.search(queries, K, exclude_ids=gone)[0]
    assert all(len(a) == K and not set(a) & set(g) for a, g in zip(after, gone))
