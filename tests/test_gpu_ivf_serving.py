"""Serving over HipIVFFlatIndex with exclusions: the resident searcher's lists
(rt_ivf_topk_lists), the index and the engine staying resident with
``exclude_ids``, and ``OnlineRecommender`` over the IVF index. Clustered
8,192 x 32 corpus of tests/_ivf_ref.py, "IVF64,Flat". The yardstick is the
unchanged bitmap path (``search_tensors(exclude_bits=...)``, an index without
``online_max_batch``): results are equal bit for bit, list for list."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _ivf_ref as ref

pytestmark = pytest.mark.gpu

NLIST, D, F, USERS = 64, 32, 10, 64
STORAGES = ["float32", "float16"]


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native, serving
    native.lib()
    return serving


def _ids(n, start=0):
    return [f"item_{i}" for i in range(start, start + n)]


def _cfg(**kw):
    cfg = {"dimension": D, "index_factory": f"IVF{NLIST},Flat", "metric": "cosine", "nprobe": 8}
    cfg.update(kw)
    return cfg


_BUILT = {}


def _built(S, fresh=False, **kw):
    """One IVF index per configuration, shared and left unchanged (``fresh``: a
    private one, for the tests that grow it or change it)."""
    key = tuple(sorted(kw.items()))
    if fresh or key not in _BUILT:
        rows, _ = ref.clustered_corpus()
        ivf = S.HipIVFFlatIndex(_cfg(**kw))
        ivf.build(rows.copy(), _ids(len(rows)))
        if fresh:
            return ivf
        _BUILT[key] = ivf
    return _BUILT[key]


def _queries(n, start=0):
    return ref.clustered_corpus()[1][start:start + n]


def _exclusions(index, q, k, seed):
    """Per query: part of its own unrestricted top-k plus random positions, of
    lengths 0, 1, 5, 166, ... (unsorted, with repeats)."""
    rng = np.random.default_rng(seed)
    top = index.search_tensors(q, k)[1].cpu().numpy()
    lens = [0, 1, 5, 166, 40, 700, 2, 64]
    out = []
    for i in range(len(q)):
        n = lens[(i + seed) % len(lens)]
        own = top[i][top[i] >= 0][: min(n, k // 2)]
        out.append(np.concatenate([own, rng.integers(0, index.current_size, n)])[: max(n, 0)].astype(np.int64))
    return out


def _bitmap_reference(index, q, k, excl):
    from rtrec_amd import kernels
    n = index.current_size
    bits = kernels.exclusion_bitmap(len(q), n, [np.unique(e) for e in excl], index._dev())
    s, p = index.search_tensors(q, k, exclude_bits=bits)
    return s.cpu().numpy(), p.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


# ---- OnlineIVFSearcher -------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_searcher_lists_equal_the_bitmap_path(S, storage):
    from rtrec_amd.serving.retrieval import OnlineIVFSearcher
    index = _built(S, storage_dtype=storage)
    s = index.online_searcher(8)
    assert isinstance(s, OnlineIVFSearcher) and s.max_exclude == 8192
    for nq in (1, 3, 8):
        for k in (10, 100):
            q = _queries(nq, 8 * nq)
            for seed in (0, 1, 2):                      # other list lengths, the same graph
                excl = _exclusions(index, q, k, seed)
                got = s.search(q, k, exclude=excl)
                assert np.shares_memory(got[0], s._h_s_np) and np.shares_memory(got[1], s._h_p_np)
                want = _bitmap_reference(index, q, k, excl)
                assert _same(got, want), (storage, nq, k, seed)
                for i, e in enumerate(excl):
                    assert not np.isin(got[1][i], e).any()
                assert (got[1] >= 0).all()              # k eligible rows exist in 8 probed lists
            assert (nq, k, 8, True) in s._graphs
    n_graphs = len(s._graphs)
    assert n_graphs == 6                                # one per (nq, k, nprobe), whatever the lists held
    q = _queries(3, 100)
    excl = _exclusions(index, q, 10, 3)
    s.search(q, 10, exclude=excl)
    assert len(s._graphs) == n_graphs
    plain = s.search(q, 10)
    assert (3, 10, 8) in s._graphs and len(s._graphs) == n_graphs + 1
    assert _same((plain[0].copy(), plain[1].copy()), tuple(a.cpu().numpy() for a in index.search_tensors(q, 10)))


def test_searcher_nprobe_eager_and_oversize(S, monkeypatch):
    index = _built(S, fresh=True)
    s = index.online_searcher(8, max_exclude=200)
    q = _queries(4, 40)
    excl = _exclusions(index, q, 10, 5)[:4]
    excl = [e[:50] for e in excl]
    first = tuple(a.copy() for a in s.search(q, 10, exclude=excl))
    assert set(s._graphs) == {(4, 10, 8, True)}
    index.nprobe = 3
    got = tuple(a.copy() for a in s.search(q, 10, exclude=excl))
    assert set(s._graphs) == {(4, 10, 8, True), (4, 10, 3, True)}
    assert _same(got, _bitmap_reference(index, q, 10, excl))
    index.nprobe = 8
    monkeypatch.setenv("RTREC_ONLINE_GRAPH", "0")
    eager = tuple(a.copy() for a in s.search(q, 10, exclude=excl))
    assert _same(eager, first) and len(s._graphs) == 2
    monkeypatch.delenv("RTREC_ONLINE_GRAPH")
    # more entries than max_exclude: the bitmap fallback, fresh arrays, the same result
    big = [np.arange(i, 8192, 97) for i in range(4)]      # 85 entries each: 340 > 200
    got = s.search(q, 10, exclude=big)
    assert not np.shares_memory(got[0], s._h_s_np)
    assert _same(got, _bitmap_reference(index, q, 10, big)) and len(s._graphs) == 2
    one = index.online_searcher(8)                        # default max_exclude takes it resident
    assert _same(one.search(q, 10, exclude=big), got)


# ---- HipIVFFlatIndex.search, RetrievalEngine ------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_index_search_with_exclude_ids_stays_resident(S, storage):
    resident = _built(S, storage_dtype=storage, online_max_batch=8)
    parent = _built(S, storage_dtype=storage)
    assert S.HipIVFFlatIndex._searcher_takes_exclude
    q = _queries(5, 30)
    for k in (10, 60):
        base_ids, _ = parent.search(q, k)
        shared = base_ids[0][:7] + ["no_such_item"]
        per_query = [row[: 3 + i] + [f"item_{17 * i}"] for i, row in enumerate(base_ids)]
        for excl in (shared, per_query):
            got = resident.search(q, k, exclude_ids=excl)
            want = parent.search(q, k, exclude_ids=excl)
            assert got == want
            for i, row in enumerate(got[0]):
                banned = set(excl if excl is shared else excl[i])
                assert len(row) == k and not banned & set(row)
        assert (5, k, 8, True) in resident._online._graphs
        allowed = _ids(8192)[::2]
        assert resident.search(q, k, allowed, exclude_ids=shared) == parent.search(q, k, allowed, exclude_ids=shared)


def test_engine_retrieve_with_exclude_ids(S):
    rows, _ = ref.clustered_corpus()
    engine = S.RetrievalEngine({"index_type": "hip_ivf", "embedding_dim": D, "top_k": 20,
                                "hip_ivf": {"index_factory": f"IVF{NLIST},Flat", "nprobe": 8, "online_max_batch": 8}})
    engine.build_index(rows.copy(), _ids(len(rows)))
    parent = _built(S, storage_dtype="float32")
    q = _queries(2, 77)
    base, _, _ = engine.retrieve(q)
    excl = [base[0][:5], base[1][:9]]
    ids, scores, metrics = engine.retrieve(q, exclude_ids=excl)
    assert (ids, scores) == parent.search(q, 20, exclude_ids=excl)
    assert all(len(r) == 20 for r in ids) and not set(ids[0]) & set(excl[0]) and not set(ids[1]) & set(excl[1])
    assert (2, 20, 8, True) in engine.index._online._graphs and not metrics["cache_hit"]


# ---- OnlineRecommender over the IVF index ---------------------------------------------
def _model(seed=0, dim=D):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    torch.manual_seed(seed)
    user = UserTower(F, embedding_dim=dim, hidden_layers=[64, 32], dropout_rate=0.2)
    item = ItemTower(6, embedding_dim=dim, hidden_layers=[16], use_content_embedding=False)
    with torch.no_grad():
        for mod in user.mlp:
            if isinstance(mod, nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
            elif isinstance(mod, nn.Linear):
                mod.bias.uniform_(-0.1, 0.1)
    return TwoTowerModel(user, item).to("cuda")


@pytest.fixture(scope="module")
def feats():
    a = np.random.default_rng(42).standard_normal((USERS, F)).astype(np.float32)
    a.setflags(write=False)
    return a


def test_recommender_accepts_the_ivf_index(S, feats):
    """The constructor refused every index but HipFlatIPIndex before."""
    from rtrec_amd.serving.retrieval import OnlineIVFSearcher
    index = _built(S, storage_dtype="float32")
    rec = S.OnlineRecommender(_model(), index)
    assert isinstance(rec._searcher, OnlineIVFSearcher) and rec._searcher.index is index
    ids, scores = rec.recommend(feats[:2], k=5)
    assert len(ids) == 2 and all(len(r) == 5 for r in ids)
    engine = S.RetrievalEngine({"index_type": "hip_ivf", "embedding_dim": D,
                                "hip_ivf": {"index_factory": f"IVF{NLIST},Flat", "nprobe": 8}})
    rows, _ = ref.clustered_corpus()
    engine.build_index(rows.copy(), _ids(len(rows)))
    assert S.OnlineRecommender(_model(), engine).recommend(feats[:2], k=5) == (ids, scores)


@pytest.mark.parametrize("storage", STORAGES)
def test_recommend_equals_search_of_embed(S, feats, storage):
    index = _built(S, storage_dtype=storage)
    table = torch.from_numpy(feats.copy()).cuda()
    rec = S.OnlineRecommender(_model(), index, user_table=table)
    for k in (10, 50):
        for nq in (1, 3, 8):
            x = feats[nq:2 * nq]
            got = rec.recommend(x, k=k)
            want = index.search(rec.embed(x).copy(), k)
            assert got == want and rec.recommend(x, k=k) == want, (storage, nq, k)
            assert (nq, k, False, False, False, 8) in rec._graphs and (nq, 0, False) in rec._graphs
            assert all(len(r) == k for r in got[0])
            uid = np.arange(nq, 2 * nq)
            assert rec.recommend(user_ids=uid, k=k) == want
    # index.nprobe is read at every call
    x = feats[:4]
    before = rec.recommend(x, k=10)
    index.nprobe = 2
    try:
        got = rec.recommend(x, k=10)
        assert got == index.search(rec.embed(x).copy(), 10)
        assert (4, 10, False, False, False, 2) in rec._graphs
    finally:
        index.nprobe = 8
    assert rec.recommend(x, k=10) == before
    # filter_ids: the 2k over-fetch
    allowed = _ids(8192)[::2]
    got = rec.recommend(x, k=30, filter_ids=allowed)
    assert got == index.search(rec.embed(x).copy(), 30, allowed)
    assert (4, 60, False, False, False, 8) in rec._graphs
    assert all(i in set(allowed) for row in got[0] for i in row)


@pytest.mark.parametrize("storage", STORAGES)
def test_recommend_with_exclusions(S, feats, storage):
    index = _built(S, storage_dtype=storage)
    table = torch.from_numpy(feats.copy()).cuda()
    rec = S.OnlineRecommender(_model(), index, user_table=table)
    rng = np.random.default_rng(3)
    k = 20
    uid = np.array([5, 9, 9, 63, 0])
    e = rec.embed(user_ids=uid).copy()
    base = index.search(e, k)[0]
    # histories: part of every user's own best items plus random ones; user 63 has none
    all_best = index.search(rec.embed(feats[:8]).copy(), k)[0] + [[] for _ in range(USERS - 8)]
    histories = [list(all_best[u][:6]) + [f"item_{i}" for i in rng.integers(0, 8192, 160)] + ["unknown"]
                 for u in range(USERS)]
    for q, u in enumerate(uid):
        histories[u] = list(base[q][: 4 + q]) + histories[u]
    histories[63] = []
    rec.set_seen(histories)
    items_shared = base[0][:3] + base[3][:3]
    items_per_row = [row[1:4 + i] for i, row in enumerate(base)]
    seen = [histories[u] for u in uid]
    for items in (items_shared, items_per_row):
        got = rec.recommend(user_ids=uid, k=k, exclude_items=items)
        assert got == index.search(e, k, exclude_ids=items)
        assert (5, k, True, True, False, 8) in rec._graphs
        both = rec.recommend(user_ids=uid, k=k, exclude_items=items, exclude_seen=True)
        per = [list(items if items is items_shared else items[q]) + seen[q] for q in range(len(uid))]
        assert both == index.search(e, k, exclude_ids=per)
        assert (5, k, True, True, True, 8) in rec._graphs
        for q, row in enumerate(both[0]):
            assert len(row) == k and not set(per[q]) & set(row)
    got = rec.recommend(user_ids=uid, k=k, exclude_seen=True)
    assert got == index.search(e, k, exclude_ids=seen)
    assert got[0][1] == got[0][2] and got[0][3] == base[3]          # the repeated user; the empty history
    assert (5, k, True, False, True, 8) in rec._graphs
    # features with per-request items
    x = feats[uid]
    assert rec.recommend(x, k=k, exclude_items=items_per_row) == index.search(e, k, exclude_ids=items_per_row)
    with pytest.raises(ValueError):
        rec.recommend(x, k=k, exclude_seen=True)


def test_recommender_follows_a_grown_index(S, feats):
    index = _built(S, fresh=True)
    rec = S.OnlineRecommender(_model(), index)
    x = feats[:3]
    e = rec.embed(x).copy()
    before = rec.recommend(x, k=10)
    unit = e / np.linalg.norm(e, axis=1, keepdims=True)
    index.add(unit.copy(), ["new_0", "new_1", "new_2"])      # each query's own direction: the new best rows
    got = rec.recommend(x, k=10)
    assert got == index.search(e, 10) and got != before
    assert [row[0] for row in got[0]] == ["new_0", "new_1", "new_2"]
    assert rec.recommend(x, k=10, exclude_items=["new_1"]) == index.search(e, 10, exclude_ids=["new_1"])


def test_recommender_over_the_flat_fallback_and_a_switch(S, feats):
    from rtrec_amd.serving.retrieval import OnlineIVFSearcher, OnlineSearcher
    rows, _ = ref.clustered_corpus()
    index = S.HipIVFFlatIndex(_cfg())
    index.build(rows[:900].copy(), _ids(900))                # under 1,024 rows: Flat
    assert index._flat is not None
    table = torch.from_numpy(feats.copy()).cuda()
    rec = S.OnlineRecommender(_model(), index, user_table=table)
    assert type(rec._searcher) is OnlineSearcher and not isinstance(rec._searcher, OnlineIVFSearcher)
    x = feats[:4]
    e = rec.embed(x).copy()
    got = rec.recommend(x, k=10)
    assert got == index.search(e, 10) and (4, 10, False) in rec._graphs
    excl = got[0][0][:4]
    assert rec.recommend(x, k=10, exclude_items=excl) == index.search(e, 10, exclude_ids=excl)
    rec.set_seen({2: got[0][2][:5]})
    assert rec.recommend(user_ids=[2], k=10, exclude_seen=True) == index.search(e[2:3], 10,
                                                                                exclude_ids=got[0][2][:5])
    index.add(rows[900:1000].copy(), _ids(100, 900))         # still Flat: the staleness path
    assert rec.recommend(x, k=10) == index.search(e, 10)
    index.build(rows.copy(), _ids(len(rows)))                # now lists: the recommender's searcher is stale
    with pytest.raises(ValueError, match="make a new one"):
        rec.recommend(x, k=10)
    rec = S.OnlineRecommender(_model(), index)
    assert rec.recommend(x, k=10) == index.search(e, 10)
    index.build(rows[:900].copy(), _ids(900))                # and back
    with pytest.raises(ValueError):
        rec.recommend(x, k=10)


def test_constructor_errors_are_unchanged(S, feats):
    index = _built(S, storage_dtype="float32")
    with pytest.raises(ValueError, match="dimension"):
        S.OnlineRecommender(_model(dim=64), index)
    l2 = S.HipFlatIPIndex({"dimension": D, "metric": "l2"})
    with pytest.raises(ValueError, match="inner-product"):
        S.OnlineRecommender(_model(), l2)
    with pytest.raises(ValueError, match="HipFlatIPIndex"):
        S.OnlineRecommender(_model(), object())
    with pytest.raises(ValueError):
        S.OnlineRecommender(_model(), S.HipIVFFlatIndex(_cfg()))   # not built: nothing to size a searcher for
