"""``HipFlatIPIndex`` with ``online_max_batch`` (the resident OnlineSearcher,
rtrec_amd/serving/retrieval.py) against the same index without it: the option
changes how a small call is served, never what it returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = 3000, 128


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native
    from rtrec_amd.serving import retrieval
    native.lib()
    return retrieval


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(42)
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((16, D)).astype(np.float32)
    ids = [f"item_{i}" for i in range(N)]
    for a in (x, q):
        a.setflags(write=False)
    return x, q, ids


def _pair(R, data, metric):
    x, _, ids = data
    off = R.HipFlatIPIndex({"dimension": D, "metric": metric})
    on = R.HipFlatIPIndex({"dimension": D, "metric": metric, "online_max_batch": 8})
    off.build(x, ids)
    on.build(x, ids)
    return off, on


@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
def test_option_on_equals_option_off(R, data, metric):
    _, q, ids = data
    off, on = _pair(R, data, metric)
    assert off._online is None and off.online_max_batch == 0
    for k in (10, 50):
        for nq in range(1, 9):
            want = off.search(q[:nq], k)
            assert on.search(q[:nq], k) == want, (metric, nq, k)
            assert (nq, k) in on._online._graphs          # the online path served it
            assert on.search(q[:nq], k) == want           # ... and its replay says the same
        # nq = 9 takes the default path
        assert on.search(q[:9], k) == off.search(q[:9], k)
        assert (9, k) not in on._online._graphs
    assert off._online is None
    # a 1-D query is one query
    got = on.search(q[3], 10)
    assert got == off.search(q[3], 10) and len(got[0]) == 1 and len(got[0][0]) == 10
    # filter_ids: k_search = 2k = 100 (online), = 200 (default path)
    allowed = ids[::2]
    n_graphs = len(on._online._graphs)
    got = on.search(q[:4], 50, filter_ids=allowed)
    assert got == off.search(q[:4], 50, filter_ids=allowed)
    assert (4, 100) in on._online._graphs and all(i in set(allowed) for row in got[0] for i in row)
    n_graphs = len(on._online._graphs)
    assert on.search(q[:4], 100, filter_ids=allowed) == off.search(q[:4], 100, filter_ids=allowed)
    assert len(on._online._graphs) == n_graphs and (4, 200) not in on._online._graphs


def test_repeated_calls_and_add(R, data):
    x, q, ids = data
    off, on = _pair(R, data, "cosine")
    a, b = on.search(q[0], 10), on.search(q[1], 10)
    assert a == off.search(q[0], 10) and b == off.search(q[1], 10) and a != b  # no stale buffer
    assert on.search(q[0], 10) == a
    rng = np.random.default_rng(7)
    # 2,000 more rows: the capacity (3,000) is exceeded, the rows move; row 3,500 is query 0 itself
    new = rng.standard_normal((2000, D)).astype(np.float32)
    new[500] = q[0]
    new_ids = [f"new_{i}" for i in range(2000)]
    ptr0, gen0 = on.index.data_ptr(), on._generation
    for idx in (off, on):
        idx.add(new, new_ids)
    assert on.index.data_ptr() != ptr0 and on._generation == gen0 + 1
    got = on.search(q[0], 10)
    assert got[0][0][0] == "new_500" and got == off.search(q[0], 10)
    assert on._online._generation == on._generation
    assert on.search(q[:8], 50) == off.search(q[:8], 50)
    # 500 more: they fit the doubled capacity, the rows stay; row 5,100 is query 1 itself
    more = rng.standard_normal((500, D)).astype(np.float32)
    more[100] = q[1]
    more_ids = [f"more_{i}" for i in range(500)]
    ptr1, gen1 = on.index.data_ptr(), on._generation
    for idx in (off, on):
        idx.add(more, more_ids)
    assert on.index.data_ptr() == ptr1 and on._generation == gen1 + 1
    got = on.search(q[1], 10)
    assert got[0][0][0] == "more_100" and got == off.search(q[1], 10)
    assert on.search(q[0], 10)[0][0][0] == "new_500"


def test_no_allocation_after_warm_up_and_eager_mode(R, data, monkeypatch):
    _, q, _ = data
    off, on = _pair(R, data, "cosine")
    s = on.online_searcher(4)
    for _ in range(3):  # warm-up: the eager first call, the capture, a replay
        on.search(q[:2], 50)
        s.search(q[:3], 10)
    want = on.search(q[:2], 50)
    assert want == off.search(q[:2], 50)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    for i in range(20):
        on.search(q[i % 8:i % 8 + 2], 50)
        s.search(q[i % 8:i % 8 + 3], 10)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    # the same sequence without the graph
    monkeypatch.setenv("RTREC_ONLINE_GRAPH", "0")
    n_graphs = len(on._online._graphs)
    assert on.search(q[:2], 50) == want
    assert on.search(q[:5], 7) == off.search(q[:5], 7)
    assert len(on._online._graphs) == n_graphs  # nothing captured in eager mode
    before3 = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(5):
        on.search(q[:2], 50)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before3
    monkeypatch.delenv("RTREC_ONLINE_GRAPH")
    assert on.search(q[:2], 50) == want


def test_searcher_returns_views_and_checks_its_arguments(R, data):
    _, q, _ = data
    off, on = _pair(R, data, "inner_product")
    s = off.online_searcher(2)
    scores, pos = s.search(q[:2], 5)
    es, ep = off.search_tensors(q[:2], 5)
    assert np.array_equal(scores, es.cpu().numpy()) and np.array_equal(pos, ep.cpu().numpy())
    # at most MAX_GRAPHS captured shapes, the oldest dropped
    s.MAX_GRAPHS = 2
    for k in (6, 7):
        s.search(q[:1], k)
    assert list(s._graphs) == [(1, 6), (1, 7)]
    assert np.array_equal(s.search(q[:2], 5)[1], ep.cpu().numpy())  # captured again, same answer
    with pytest.raises(ValueError):
        s.search(q[:3], 5)          # more than max_batch
    with pytest.raises(ValueError):
        s.search(q[:1], 129)
    with pytest.raises(ValueError):
        s.search(q[:1, :64], 5)     # wrong dimension
    with pytest.raises(ValueError):
        off.online_searcher(9)
    with pytest.raises(ValueError):
        R.HipFlatIPIndex({"dimension": D}).online_searcher(1).search(q[:1], 5)  # not built


def test_half_storage_is_served(R, data):
    """16-bit storage: the online scores are the fp32 chain over the stored
    rows (the default path's are MFMA sums), so the check is against the oracle."""
    from oracle import flat_ip as orc
    x, q, ids = data
    on = R.HipFlatIPIndex({"dimension": D, "metric": "inner_product", "storage_dtype": "float16",
                           "online_max_batch": 8})
    on.build(x, ids)
    rs, ri = orc.flat_ip_search(q[:4].astype(np.float16), x.astype(np.float16), 20, nthreads=4)
    got_ids, got_scores = on.search(q[:4], 20)
    assert got_ids == [[ids[p] for p in row] for row in ri]
    assert got_scores == [[float(v) for v in row] for row in rs]


def test_load_of_another_shape_drops_the_searcher(R, data, tmp_path):
    """load() may change the dimension and the metric: the index's own searcher
    is dropped with them, a searcher the caller holds refuses to go on."""
    x, q, ids = data
    small = R.HipFlatIPIndex({"dimension": 64, "metric": "inner_product"})
    small.build(x[:500, :64], ids[:500])
    small.save(str(tmp_path / "small"))
    flat_l2 = R.HipFlatIPIndex({"dimension": D, "metric": "l2"})
    flat_l2.build(x[:500], ids[:500])
    flat_l2.save(str(tmp_path / "l2"))
    off, on = _pair(R, data, "inner_product")
    held = on.online_searcher(2)
    assert on.search(q[:2], 10) == off.search(q[:2], 10) and on._online is not None
    held.search(q[:1], 5)
    on.load(str(tmp_path / "small"))
    assert on._online is None and on.dimension == 64
    assert on.search(q[:2, :64], 10) == small.search(q[:2, :64], 10)
    assert on._online is not None and on._online._h_q.shape[1] == 64
    with pytest.raises(ValueError):
        held.search(q[:1, :64], 5)
    on.load(str(tmp_path / "l2"))   # an L2 index: the online path must not serve it
    assert on._l2 and on._online is None
    assert on.search(q[:2], 10) == flat_l2.search(q[:2], 10)
    assert on._online is None


def test_configuration_errors(R):
    with pytest.raises(ValueError):
        R.HipFlatIPIndex({"dimension": D, "metric": "l2", "online_max_batch": 4})
    with pytest.raises(ValueError):
        R.HipFlatIPIndex({"dimension": D, "online_max_batch": 9})
    with pytest.raises(ValueError):
        R.HipFlatIPIndex({"dimension": D, "online_max_batch": -1})
    assert R.HipFlatIPIndex({"dimension": D, "metric": "l2"}).online_max_batch == 0


def test_engine_route(R, data):
    x, q, ids = data
    base = {"index_type": "hip_flat", "embedding_dim": D, "top_k": 50}
    eng_off = R.RetrievalEngine(dict(base))
    eng_on = R.RetrievalEngine(dict(base, hip_flat={"online_max_batch": 8}))
    assert eng_on.index.online_max_batch == 8 and eng_off.index.online_max_batch == 0
    for eng in (eng_off, eng_on):
        eng.build_index(x, ids)
    for query in (q[0], q[:1], q[:8]):
        i_off, s_off, m_off = eng_off.retrieve(query, use_cache=False)
        i_on, s_on, m_on = eng_on.retrieve(query, use_cache=False)
        assert i_on == i_off and s_on == s_off
        assert set(m_on) == set(m_off) and m_on["num_results"] == m_off["num_results"]
        assert m_on["avg_score"] == m_off["avg_score"] and m_on["cache_hit"] is False
    assert (1, 50) in eng_on.index._online._graphs and (8, 50) in eng_on.index._online._graphs
    assert eng_on.get_metrics()["total_queries"] == 3
