"""``OnlineRecommender`` (rtrec_amd/serving/online.py): user features or user ids
in, recommendation lists out, one graph replay and one synchronise. The chain
after the embedding is the online searcher's, so its lists equal
``index.search(embed(x), k)`` exactly; the embedding meets the fp32-class bar
against ``get_user_embeddings``; end to end it is checked against the oracle at
every rank that is not a near tie."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N, D, F, USERS = 3000, 128, 10, 64


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native, serving
    native.lib()
    return serving


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(42)
    x = rng.standard_normal((N, D)).astype(np.float32)
    ids = [f"item_{i}" for i in range(N)]
    feats = rng.standard_normal((USERS, F)).astype(np.float32)
    for a in (x, feats):
        a.setflags(write=False)
    return x, ids, feats


def _model(seed=0, in_dim=F, hidden=(64, 32), dev="cuda"):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    torch.manual_seed(seed)
    user = UserTower(in_dim, embedding_dim=D, hidden_layers=list(hidden), dropout_rate=0.2)
    item = ItemTower(6, embedding_dim=D, hidden_layers=[16], use_content_embedding=False)
    with torch.no_grad():
        for mod in user.mlp:
            if isinstance(mod, nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
            elif isinstance(mod, nn.Linear):
                mod.bias.uniform_(-0.1, 0.1)
    return TwoTowerModel(user, item).to(dev)


def _oracle_embed(model, feats):
    from oracle import two_tower as orc
    state = {k: v.detach().cpu().clone() for k, v in model.user_tower.state_dict().items()}
    with torch.no_grad():
        return orc.tower_forward(state, torch.from_numpy(np.ascontiguousarray(feats)), train=False).numpy()


def _index(S, data, metric="cosine", storage="float32"):
    x, ids, _ = data
    index = S.HipFlatIPIndex({"dimension": D, "metric": metric, "storage_dtype": storage, "online_max_batch": 8})
    index.build(x, ids)
    return index


@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
def test_recommend_equals_search_of_embed(S, data, metric, storage):
    _, ids, feats = data
    index = _index(S, data, metric, storage)
    rec = S.OnlineRecommender(_model(), index)
    for k in (10, 50):
        for nq in range(1, 9):
            x = feats[nq:2 * nq]
            got = rec.recommend(x, k=k)
            want = index.search(rec.embed(x).copy(), k)
            assert got == want, (metric, storage, nq, k)
            assert (nq, k, False) in rec._graphs and (nq, 0, False) in rec._graphs
            assert rec.recommend(x, k=k) == want            # the replay says the same
            assert len(got[0]) == nq and all(len(r) == k for r in got[0])
    # the reference's feature dict, a tensor and a single row
    one = rec.recommend({"numerical": torch.from_numpy(feats[:1].copy()), "categorical": {}}, k=10)
    assert one == rec.recommend(feats[0], k=10) == rec.recommend(feats[:1], k=10)


def test_user_ids_path_is_bit_equal_to_the_gathered_rows(S, data):
    _, _, feats = data
    index = _index(S, data)
    table = torch.from_numpy(feats.copy()).cuda()
    rec = S.OnlineRecommender(_model(), index, user_table=table)
    for ids in ([5], [63, 0, 17], list(range(8, 16))):
        by_id = rec.embed(user_ids=ids).copy()
        by_row = rec.embed(feats[ids]).copy()
        assert np.array_equal(by_id, by_row)
        assert rec.recommend(user_ids=np.asarray(ids), k=10) == rec.recommend(feats[ids], k=10)
        assert (len(ids), 10, True) in rec._graphs
    with pytest.raises(IndexError):
        rec.embed(user_ids=[0, USERS])
    with pytest.raises(IndexError):
        rec.recommend(user_ids=[-1], k=5)
    with pytest.raises(ValueError):
        rec.embed(feats[:1], user_ids=[0])      # both
    with pytest.raises(ValueError):
        rec.embed()                             # neither
    with pytest.raises(ValueError):
        S.OnlineRecommender(_model(), index).embed(user_ids=[0])   # no table


def test_filter_and_the_fall_back(S, data):
    _, ids, feats = data
    index = _index(S, data)
    rec = S.OnlineRecommender(_model(), index)
    allowed = ids[::2]
    x = feats[:4]
    e = rec.embed(x).copy()
    got = rec.recommend(x, k=50, filter_ids=allowed)                 # k_search = 100: resident
    assert got == index.search(e, 50, allowed) and (4, 100, False) in rec._graphs
    assert all(i in set(allowed) for row in got[0] for i in row)
    assert set(rec._graphs) == {(4, 0, False), (4, 100, False)}
    assert rec.recommend(x, k=100, filter_ids=allowed) == index.search(e, 100, allowed)   # k_search = 200
    x9 = feats[:9]
    e9 = rec.embed(x9).copy()                                        # nq = 9: embedded in chunks
    assert e9.shape == (9, D) and np.array_equal(e9[:4], e)
    assert rec.recommend(x9, k=10) == index.search(e9, 10)
    # the fall-back captured no search graph: only the embed graphs of the chunks (8 and 1 rows) are new
    assert set(rec._graphs) == {(4, 0, False), (4, 100, False), (8, 0, False), (1, 0, False)}


def test_embed_meets_the_fp32_class_bar(S, data):
    _, _, feats = data
    model = _model(hidden=(512, 256, 128)).eval()    # the service-default tower
    rec = S.OnlineRecommender(model, _index(S, data))
    x = feats[:8]
    with torch.no_grad():
        want = model.get_user_embeddings({"numerical": torch.from_numpy(x.copy()).cuda(), "categorical": {}})
    got = rec.embed(x)
    err = np.abs(got - want.cpu().numpy()).max()
    print(f"embed vs get_user_embeddings: max abs err {err:.3e}")
    assert err <= 2e-6, err
    # eval semantics regardless of model.training (dropout 0.2 and batch statistics would show)
    model.train()
    assert np.array_equal(rec.embed(x), got)
    model.eval()


def test_end_to_end_against_the_oracle_without_hiding_near_ties(S, data):
    from oracle import flat_ip as orc
    x, ids, feats = data
    model = _model()
    rec = S.OnlineRecommender(model, _index(S, data))
    xn = x.copy()
    orc.normalize_L2(xn)                 # the index's build step (faiss.normalize_L2)
    k, nq = 50, 8
    u_ref = np.ascontiguousarray(_oracle_embed(model, feats[:nq]))
    orc.normalize_L2(u_ref)              # ... and its search step
    u_gpu = rec.embed(feats[:nq]).copy()
    delta = np.linalg.norm(u_gpu.astype(np.float64) - u_ref.astype(np.float64), axis=1)
    rs, ri = orc.flat_ip_search(u_ref, xn, k + 1, nthreads=4)
    got_ids, _ = rec.recommend(feats[:nq], k=k)
    compared = 0
    for q in range(nq):
        s = rs[q].astype(np.float64)
        gap_next = s[:k] - s[1:k + 1]                               # to the rank below (rank k: the first one out)
        gap_prev = np.concatenate([[np.inf], s[:k - 1] - s[1:k]])   # to the rank above
        clear = (gap_next > 2 * delta[q]) & (gap_prev > 2 * delta[q])
        for r in np.nonzero(clear)[0]:
            assert got_ids[q][r] == ids[ri[q, r]], (q, r)
        compared += int(clear.sum())
    print(f"compared {compared} of {k * nq} ranks, delta max {delta.max():.3e}")
    assert compared >= 0.9 * k * nq, compared


def test_staleness_index_and_model(S, data):
    x, ids, feats = data
    index = _index(S, data)
    model = _model()
    rec = S.OnlineRecommender(model, index)
    q = feats[:3]
    before = rec.recommend(q, k=10)
    # 2,000 more rows: the capacity is exceeded, the rows move
    rng = np.random.default_rng(7)
    new = rng.standard_normal((2000, D)).astype(np.float32)
    new[500] = rec.embed(q)[0]
    ptr0 = index.index.data_ptr()
    index.add(new, [f"new_{i}" for i in range(2000)])
    assert index.index.data_ptr() != ptr0
    got = rec.recommend(q, k=10)
    assert got[0][0][0] == "new_500" and got == index.search(rec.embed(q).copy(), 10) and got != before
    # other weights in place, no refresh(): the next embed is the oracle's on the NEW weights
    old = rec.embed(q).copy()
    other = _model(seed=5, dev="cpu")
    model.load_state_dict(other.state_dict())
    ref_new = _oracle_embed(other, q)
    now = rec.embed(q).copy()
    assert np.abs(now - ref_new).max() <= 1e-4 * np.abs(ref_new).max()
    assert np.abs(now - old).max() > 1e-2
    assert rec.recommend(q, k=10) == index.search(now, 10)
    # the tensors re-allocated (what model.to(...) does): refresh() makes it right again
    third = _model(seed=9, dev="cpu")
    model.load_state_dict(third.state_dict())
    for t in list(model.parameters()) + list(model.buffers()):
        t.data = t.data.clone()
    rec.refresh()
    ref3 = _oracle_embed(third, q)
    assert np.abs(rec.embed(q) - ref3).max() <= 1e-4 * np.abs(ref3).max()
    assert rec.recommend(q, k=10) == index.search(rec.embed(q).copy(), 10)


def test_no_allocation_after_warm_up_and_eager_mode(S, data, monkeypatch):
    _, _, feats = data
    index = _index(S, data)
    rec = S.OnlineRecommender(_model(), index)
    for _ in range(3):
        want = rec.recommend(feats[:2], k=50)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    for i in range(10):
        rec.recommend(feats[i:i + 2], k=50)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    monkeypatch.setenv("RTREC_ONLINE_GRAPH", "0")
    n_graphs = len(rec._graphs)
    assert rec.recommend(feats[:2], k=50) == want
    assert rec.recommend(feats[:5], k=7) == index.search(rec.embed(feats[:5]).copy(), 7)
    assert len(rec._graphs) == n_graphs


def test_errors(S, data):
    x, ids, feats = data
    index = _index(S, data)
    model = _model()
    with pytest.raises(ValueError, match="dimension"):
        S.OnlineRecommender(model, S.HipFlatIPIndex({"dimension": 64}))
    with pytest.raises(ValueError, match="inner-product"):
        S.OnlineRecommender(model, S.HipFlatIPIndex({"dimension": D, "metric": "l2"}))
    with pytest.raises(ValueError):
        S.OnlineRecommender(model, index, max_batch=0)
    unbuilt = S.OnlineRecommender(model, S.HipFlatIPIndex({"dimension": D}))
    assert unbuilt.embed(feats[:1]).shape == (1, D)             # embed needs no corpus
    with pytest.raises(ValueError, match="Index not built yet"):
        unbuilt.recommend(feats[:1], k=5)
    rec = S.OnlineRecommender(model, index)
    with pytest.raises(ValueError):
        rec.recommend(feats[:1, :4], k=5)                         # wrong feature width
    with pytest.raises(ValueError):
        rec.recommend({"numerical": feats[:1], "categorical": {"g": torch.zeros(1, dtype=torch.long)}}, k=5)
    # a RetrievalEngine whose index is a HipFlatIPIndex
    eng = S.RetrievalEngine({"index_type": "hip_flat", "embedding_dim": D, "top_k": 10})
    eng.build_index(x, ids)
    via_engine = S.OnlineRecommender(model, eng)
    assert via_engine.recommend(feats[:2], k=10) == rec.recommend(feats[:2], k=10)
