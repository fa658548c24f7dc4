"""The MMR re-rank through the serving layers: ``search(..., mmr_lambda=...)`` of
the Flat and IVF indexes (resident and not), ``OnlineRecommender.recommend`` and
the offline evaluation. A re-ranked search is held to the fp64 reference of
_mmr_ref applied to the SAME index's plain ``search(q, k=100)`` output
(``check_trace``); paths that see the same candidates are held to each other bit
for bit, which the kernel's determinism contract promises."""
import numpy as np
import pytest
import torch

import _mmr_ref as mref

pytestmark = pytest.mark.gpu

D = 64
N_FLAT, N_IVF, NLIST = 2000, 4096, 32
CATS = ["a", "b", "c"]


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native, serving
    native.lib()
    return serving


@pytest.fixture(scope="module")
def corpus():
    """The clustered corpus of test_gpu_mmr.py, once: rows, string ids, queries, categories."""
    rows, _ = mref.clustered(21, N_IVF, D)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((16, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cats = [[CATS[p % 3]] if p % 7 else [] for p in range(N_IVF)]
    rows, q = rows.astype(np.float32), q.astype(np.float32)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, [f"i{p}" for p in range(N_IVF)], q, cats


def _build(S, corpus, kind, n, metric="cosine", storage="float32", online=8, nprobe=8, categories=False):
    rows, ids, _, cats = corpus
    cfg = {"dimension": D, "metric": metric, "storage_dtype": storage, "online_max_batch": online}
    if categories:
        cfg["categories"] = CATS
    if kind == "flat":
        index = S.HipFlatIPIndex(cfg)
    else:
        cfg.update(index_factory=f"IVF{NLIST},Flat", nprobe=nprobe)
        index = (S.HipIVFFlatIndex if kind == "ivf" else S.retrieval.HipMutableIVFFlatIndex)(cfg)
    kw = {"item_categories": cats[:n]} if categories else {}
    scale = 1.0 if metric == "cosine" else np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
    index.build(rows[:n] * scale, ids[:n], **kw)
    return index


def _pos(ids):
    return np.array([int(i[1:]) for i in ids], dtype=np.int64)


def _check_against_plain(index, q, k, lam, **kw):
    """search(q, k, mmr_lambda=lam) against the reference over search(q, 100)'s own output."""
    got_ids, got_scores = index.search(q, k, mmr_lambda=lam, **kw)
    cand_ids, cand_scores = index.search(q, 100, **kw)
    stored = index.vectors().astype(np.float64)
    normalize = index.metric != "cosine"
    for r in range(len(q)):
        assert len(got_ids[r]) == k
        mref.check_trace(np.array(cand_scores[r], np.float32), _pos(cand_ids[r]), stored, k, lam, normalize,
                         np.array(got_scores[r], np.float32), _pos(got_ids[r]))
    return got_ids, got_scores


# ---- search ----
@pytest.mark.parametrize("storage", ["float16", "float32"])
@pytest.mark.parametrize("kind,n", [("flat", N_FLAT), ("ivf", N_IVF), ("ivf_mutable", N_IVF)])
def test_search_is_the_reference_over_the_plain_candidates(S, corpus, kind, n, storage):
    index = _build(S, corpus, kind, n, storage=storage)
    q = corpus[2]
    small, _ = _check_against_plain(index, q[:3], 10, 0.5)            # resident: nq within online_max_batch
    searcher = index._online
    assert searcher is not None and any(key[-2:] == ("mmr", 10) for key in searcher._graphs)
    assert any("mmr" not in key for key in searcher._graphs)          # the plain k = 100 call: today's key
    large, _ = _check_against_plain(index, q[:12], 10, 0.5)           # above it: search_tensors + the kernel
    if storage == "float32" or kind != "flat":   # (the Flat batch kernel's float16 scores differ in the last bits)
        assert large[:3] == small                                     # the same candidates: the same lists
    plain, _ = index.search(q[:3], 10)
    assert all(a != b for a, b in zip(small, plain))                  # lambda = 0.5 reorders this corpus
    ident, ident_s = index.search(q[:3], 10, mmr_lambda=1.0)
    assert (ident, ident_s) == index.search(q[:3], 10)                # lambda = 1: the plain top-k
    # mmr_candidates: the candidates are the plain top-40
    got, got_s = index.search(q[:2], 5, mmr_lambda=0.3, mmr_candidates=40)
    c_ids, c_s = index.search(q[:2], 40)
    for r in range(2):
        mref.check_trace(np.array(c_s[r], np.float32), _pos(c_ids[r]), index.vectors().astype(np.float64), 5, 0.3,
                         False, np.array(got_s[r], np.float32), _pos(got[r]))


def test_inner_product_metric_normalises(S, corpus):
    index = _build(S, corpus, "flat", N_FLAT, metric="inner_product", storage="float32")
    q = corpus[2]
    norms = np.linalg.norm(index.vectors(), axis=1)
    assert norms.min() < 0.6 and norms.max() > 1.9                    # the rows are not unit-norm
    a, _ = _check_against_plain(index, q[:4], 10, 0.5)
    b, _ = _check_against_plain(index, q[:10], 10, 0.5)
    assert b[:4] == a


def test_not_resident_without_online_max_batch(S, corpus):
    index = _build(S, corpus, "ivf", N_IVF, online=0)
    _check_against_plain(index, corpus[2][:2], 10, 0.7)
    assert index._online is None


@pytest.mark.parametrize("storage", ["float16", "float32"])
@pytest.mark.parametrize("kind", ["ivf", "ivf_mutable"])
def test_every_list_probed_is_the_flat_rerank_bit_for_bit(S, corpus, kind, storage):
    """The IVF lists, resident (nq = 4) and not (nq = 12), against the Flat index's
    RESIDENT re-ranked lists, 8 queries a call: both scans score by the same fmaf
    chain, so the candidates are the same bits and so must the results be. For
    float32 rows the Flat index's non-resident call is that chain too and is
    compared as well; for float16 rows its batch kernel scores through MFMA and
    differs from the chain in the last bits (test_gpu_ivf_index.py), so there its
    candidates are not the IVF index's and it is no reference for bits."""
    flat = _build(S, corpus, "flat", N_IVF, storage=storage)
    ivf = _build(S, corpus, kind, N_IVF, storage=storage, nprobe=NLIST)
    q = corpus[2]
    for lam in (0.0, 0.5):
        want_ids, want_scores = [], []
        for a in range(0, 12, 8):                                     # the Flat index's online path
            ids, scores = flat.search(q[a:min(a + 8, 12)], 10, mmr_lambda=lam)
            want_ids += ids
            want_scores += scores
        for nq in (4, 12):                                            # resident and not
            got_ids, got_scores = ivf.search(q[:nq], 10, mmr_lambda=lam)
            assert got_ids == want_ids[:nq], (lam, nq)
            assert got_scores == want_scores[:nq], (lam, nq)
        if storage == "float32":
            assert flat.search(q[:12], 10, mmr_lambda=lam) == (want_ids, want_scores), lam


# ---- composition ----
@pytest.mark.parametrize("kind,n", [("flat", N_FLAT), ("ivf_mutable", N_IVF)])
def test_composes_with_exclusions_and_category_filters(S, corpus, kind, n):
    index = _build(S, corpus, kind, n, categories=True, nprobe=16)
    q, cats = corpus[2], corpus[3]
    for nq in (2, 10):
        plain, _ = index.search(q[:nq], 30, filter_categories=["a", "b"])
        excl = [ids[:15:2] for ids in plain]                          # per query: every other of its best
        kw = dict(exclude_ids=excl, filter_categories=["a", "b"])
        got, _ = _check_against_plain(index, q[:nq], 10, 0.5, **kw)
        for r in range(nq):
            assert len(got[r]) == 10 and not set(got[r]) & set(excl[r])
            assert all(cats[int(i[1:])] and cats[int(i[1:])][0] in ("a", "b") for i in got[r])


# ---- the mutable IVF index and the recommender ----
def _model(in_dim=10):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    torch.manual_seed(0)
    user = UserTower(in_dim, embedding_dim=D, hidden_layers=[32], dropout_rate=0.2)
    item = ItemTower(6, embedding_dim=D, hidden_layers=[16], use_content_embedding=False)
    return TwoTowerModel(user, item).cuda()


@pytest.mark.parametrize("kind,n", [("flat", N_FLAT), ("ivf", N_IVF)])
def test_recommender_equals_search_of_embed(S, corpus, kind, n):
    index = _build(S, corpus, kind, n, storage="float16")
    rec = S.OnlineRecommender(_model(), index)
    feats = np.random.default_rng(9).standard_normal((12, 10)).astype(np.float32)
    x = feats[:3]
    got = rec.recommend(x, k=10, mmr_lambda=0.5)
    assert got == index.search(rec.embed(x).copy(), 10, mmr_lambda=0.5)
    assert got[0] != rec.recommend(x, k=10)[0] and all(len(r) == 10 for r in got[0])
    graphs = len(rec._graphs)
    assert sum(1 for key in rec._graphs if key[-2:] == ("mmr", 10)) == 1
    for lam in (0.2, 0.9, 1.0):                                       # lambda is data: no new graph
        assert rec.recommend(x, k=10, mmr_lambda=lam) == index.search(rec.embed(x).copy(), 10, mmr_lambda=lam)
    assert len(rec._graphs) == graphs
    assert rec.recommend(x, k=10, mmr_lambda=1.0) == rec.recommend(x, k=10)
    # above max_batch: embedded in chunks, index.search, the same lists
    big = rec.recommend(feats, k=10, mmr_lambda=0.5)
    assert big == index.search(rec.embed(feats).copy(), 10, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="filter_ids together with mmr_lambda"):
        rec.recommend(x, k=10, filter_ids=["i1"], mmr_lambda=0.5)


def test_mutable_update_keeps_the_graphs_and_is_read_by_the_next_call(S, corpus):
    index = _build(S, corpus, "ivf_mutable", N_IVF, nprobe=NLIST)
    rec = S.OnlineRecommender(_model(), index)
    x = np.random.default_rng(4).standard_normal((2, 10)).astype(np.float32)
    before = rec.recommend(x, k=10, mmr_lambda=0.5)
    graphs, generation = len(rec._graphs), index._generation
    # the second choice of user 0 becomes a copy of the first: its row changes (and may change lists)
    first, second = before[0][0][0], before[0][0][1]
    vec = index.vectors()
    index.update(vec[int(first[1:])][None, :].copy(), [second])
    assert index._generation == generation
    after = rec.recommend(x, k=10, mmr_lambda=0.5)
    assert len(rec._graphs) == graphs and after != before
    e = rec.embed(x).copy()
    cand_ids, cand_s = index.search(e, 100)
    stored = index.vectors().astype(np.float64)
    assert np.allclose(stored[int(second[1:])], stored[int(first[1:])], rtol=0, atol=1e-6)   # renormalised once more
    for r in range(2):
        mref.check_trace(np.array(cand_s[r], np.float32), _pos(cand_ids[r]), stored, 10, 0.5, False,
                         np.array(after[1][r], np.float32), _pos(after[0][r]))
    # the copy now has similarity 1 to the first choice: it is no longer chosen second
    assert after[0][0][0] in (first, second) and after[0][0][1] not in (first, second)


# ---- the metric it moves, and the evaluation ----
def test_diversity_at_10_rises(S, corpus):
    from rtrec_amd.evaluation import list_metrics_tensors
    index = _build(S, corpus, "flat", N_FLAT)
    q = torch.from_numpy(corpus[2].copy())
    s100, p100 = index.search_tensors(q, 100)
    s10, p10 = index.mmr_rerank_tensors(s100, p100, 10, 0.5)
    emb = index.index[: index.current_size]
    plain = list_metrics_tensors(p100[:, :10].contiguous(), [10], item_embeddings=emb).diversity[10]
    mmr = list_metrics_tensors(p10, [10], item_embeddings=emb).diversity[10]
    assert mmr > plain, (plain, mmr)     # the fp64 reference gains 0.028 or more per list on this recipe


def test_evaluation_reranks_the_top_candidates():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import load_golden
    from rtrec_amd.evaluation.metrics import csr_from_sets
    from rtrec_amd.evaluation.offline import recommend_tensors
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    g = load_golden("movielens_tiny")
    uf = torch.from_numpy(g["user_features"].astype(np.float32)).cuda()
    mf = torch.from_numpy(g["movie_features"].astype(np.float32)).cuda()
    torch.manual_seed(2)
    model = TwoTowerModel(UserTower(uf.shape[1], embedding_dim=32, hidden_layers=[16]),
                          ItemTower(mf.shape[1], embedding_dim=32, hidden_layers=[16],
                                    use_content_embedding=False)).cuda().eval()
    train = [[int(x) for x in row if x >= 0] for row in g["positives"]]
    t_off, t_items = csr_from_sets(train, uf.device)
    users = torch.arange(uf.shape[0], dtype=torch.int64, device=uf.device)
    top_k, n_items = 5, int(mf.shape[0])
    args = (model, uf, mf, users, t_off, t_items)
    cs, ci = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=n_items))      # the default candidates: all 15
    gs, gi = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=top_k, mmr_lambda=0.5))
    with torch.no_grad():
        emb = model.get_item_embeddings({"numerical": mf, "categorical": {}}).double().cpu().numpy()
    assert gi.shape == (uf.shape[0], top_k)
    for u in range(uf.shape[0]):
        assert set(gi[u][gi[u] >= 0]) <= set(ci[u][ci[u] >= 0]) and not set(gi[u]) & set(train[u])
        mref.check_trace(cs[u], ci[u], emb, top_k, 0.5, True, gs[u], gi[u])
    # an explicit candidate count, and lambda = 1 is the plain evaluation
    c8s, c8i = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=8))
    g8s, g8i = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=top_k, mmr_lambda=0.25, mmr_candidates=8))
    for u in range(uf.shape[0]):
        mref.check_trace(c8s[u], c8i[u], emb, top_k, 0.25, True, g8s[u], g8i[u])
    ps, pi = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=top_k))
    is_, ii = (t.cpu().numpy() for t in recommend_tensors(*args, top_k=top_k, mmr_lambda=1.0))
    assert np.array_equal(ii, pi) and np.array_equal(is_.view(np.uint32), ps.view(np.uint32))
    with pytest.raises(ValueError, match="top_k <= mmr_candidates <= 128"):
        recommend_tensors(*args, top_k=top_k, mmr_lambda=0.5, mmr_candidates=4)
