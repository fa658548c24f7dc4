"""HipIVFFlatIndex and its resident searcher on the clustered 8,192 x 32 corpus
of tests/_ivf_ref.py with "IVF64,Flat". The exact Flat index on the same GPU is
the yardstick: nprobe = nlist must equal it id for id and score for score, and
fewer probes must reach its results with the recall the numpy reference shows
the lists allow (tests/test_ivf_ref_cpu.py: 1.000 at nprobe = 8)."""
import numpy as np
import pytest
import torch

import _ivf_ref as ref

pytestmark = pytest.mark.gpu

NLIST, D = 64, 32


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native
    from rtrec_amd.serving import retrieval
    native.lib()
    return retrieval


def _ids(n, start=0):
    return [f"item_{i}" for i in range(start, start + n)]


def _cfg(**kw):
    cfg = {"dimension": D, "index_factory": f"IVF{NLIST},Flat", "metric": "cosine", "nprobe": 8}
    cfg.update(kw)
    return cfg


_BUILT = {}


def _built(R, **kw):
    """One IVF index and one Flat index per configuration, shared and left unchanged."""
    key = tuple(sorted(kw.items()))
    if key not in _BUILT:
        rows, _ = ref.clustered_corpus()
        ivf = R.HipIVFFlatIndex(_cfg(**kw))
        ivf.build(rows.copy(), _ids(len(rows)))
        flat = R.HipFlatIPIndex({"dimension": D, "metric": kw.get("metric", "cosine"),
                                 "storage_dtype": kw.get("storage_dtype", "float32"), "online_max_batch": 8})
        flat.build(rows.copy(), _ids(len(rows)))
        _BUILT[key] = (ivf, flat)
    return _BUILT[key]


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def test_recall_at_nprobe_8(R):
    """recall@10 >= 0.95 at nprobe = 8 against HipFlatIPIndex (the numpy reference
    measures 1.000; the margin is for assignment ties that differ between fp32
    and fp64)."""
    ivf, flat = _built(R)
    _, queries = ref.clustered_corpus()
    _, want = _np(flat.search_tensors(queries, 10))
    _, got = _np(ivf.search_tensors(queries, 10))
    r = ref.recall_at_k(got, want)
    print(f"recall@10 at nprobe=8: {r:.4f}")
    assert r >= 0.95


@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_every_list_probed_equals_flat(R, metric, storage):
    """nprobe = nlist: the id lists and the float scores of HipFlatIPIndex, for all
    64 queries, through the Flat index's online path (``OnlineSearcher``, 8
    queries a call), whose scores are by contract the fmaf chain rt_ivf_topk
    computes. For float32 rows the batch search over the 64 queries is that
    chain too and is compared as well; for float16 rows the batch kernel
    scores through MFMA and differs from the chain in the last bits (measured
    here: up to 2 ulp, which reorders near-ties), so it is no reference for
    bits."""
    ivf, flat = _built(R, metric=metric, storage_dtype=storage)
    _, queries = ref.clustered_corpus()
    q = queries[:64] * (1.0 if metric == "cosine" else 3.0)
    online = flat.online_searcher(8)
    for k in (10, 100):
        ws, wi = _np(flat.search_tensors(q, k))
        gs, gi = _np(ivf.search_tensors(q, k, nprobe=NLIST))
        if storage == "float32":
            assert np.array_equal(gi, wi)
            assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        for a in range(0, 64, 8):
            os_, oi = online.search(q[a:a + 8], k)
            assert np.array_equal(gi[a:a + 8], oi)
            assert np.array_equal(gs[a:a + 8].view(np.uint32), os_.view(np.uint32))
    ids_f, sc_f = flat.search(q[:5], 10)    # online_max_batch = 8: the online path
    ivf.nprobe = NLIST
    try:
        ids_i, sc_i = ivf.search(q[:5], 10)
    finally:
        ivf.nprobe = 8
    assert ids_i == ids_f and sc_i == sc_f


def test_balance_and_layout(R):
    """Every row is in exactly one list, row_pos is a permutation, the stored rows
    are the prepared rows of their positions in original order within a list, and
    no list exceeds 8 n / nlist (a sanity bound; the reference's longest was 399)."""
    ivf, flat = _built(R)
    n = ivf.current_size
    off = ivf.list_offsets.cpu().numpy()
    pos = ivf.row_pos.cpu().numpy()
    assign = ivf.assign.cpu().numpy()
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all() and len(off) == NLIST + 1
    assert np.array_equal(np.sort(pos), np.arange(n))
    assert np.diff(off).max() <= 8 * n // NLIST and ivf.max_list_rows == np.diff(off).max()
    for l in range(NLIST):
        p = pos[off[l]:off[l + 1]]
        assert (assign[p] == l).all() and (np.diff(p) > 0).all()
    assert np.array_equal(ivf.vectors(), flat.vectors())
    assert ivf.index.shape[0] == n          # stored once


def test_determinism(R):
    rows, _ = ref.clustered_corpus()
    a, _ = _built(R)
    b = R.HipIVFFlatIndex(_cfg())
    b.build(rows.copy(), _ids(len(rows)))
    for name in ("centroids", "list_offsets", "row_pos", "assign", "index"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    c = R.HipIVFFlatIndex(_cfg(seed=99))
    c.build(rows.copy(), _ids(len(rows)))
    assert not torch.equal(a.centroids, c.centroids)


def test_small_corpus_falls_back_to_flat(R):
    rows, queries = ref.clustered_corpus()
    small = rows[:500].copy()
    ivf = R.HipIVFFlatIndex(_cfg())
    ivf.build(small, _ids(500))
    flat = R.HipFlatIPIndex({"dimension": D})
    flat.build(small, _ids(500))
    assert ivf.centroids is None and ivf.current_size == 500
    assert ivf.search(queries[:4], 10) == flat.search(queries[:4], 10)
    gs, gi = _np(ivf.search_tensors(queries[:4], 10))
    ws, wi = _np(flat.search_tensors(queries[:4], 10))
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws)
    assert isinstance(ivf.online_searcher(), R.OnlineSearcher)


def test_add(R):
    """After adding 300 rows, searching at nprobe = nlist equals a Flat index
    given the same build + add; the lists stay a partition in original order."""
    rows, queries = ref.clustered_corpus()
    n0 = len(rows) - 300
    ivf = R.HipIVFFlatIndex(_cfg())
    flat = R.HipFlatIPIndex({"dimension": D})
    for idx in (ivf, flat):
        idx.build(rows[:n0].copy(), _ids(n0))
        idx.add(rows[n0:].copy(), _ids(300, n0))
    assert ivf.current_size == len(rows)
    pos = ivf.row_pos.cpu().numpy()
    assert np.array_equal(np.sort(pos), np.arange(len(rows)))
    assert np.array_equal(ivf.vectors(), flat.vectors())
    ws, wi = _np(flat.search_tensors(queries[:64], 20))
    gs, gi = _np(ivf.search_tensors(queries[:64], 20, nprobe=NLIST))
    assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    ids, _ = ivf.search(rows[-1], 1)
    assert ids == [[f"item_{len(rows) - 1}"]]


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_save_load_round_trip(R, tmp_path, storage):
    ivf, _ = _built(R, storage_dtype=storage)
    _, queries = ref.clustered_corpus()
    ivf.save(str(tmp_path / "idx"))
    other = R.HipIVFFlatIndex(_cfg(storage_dtype=storage))
    other.load(str(tmp_path / "idx"))
    for name in ("centroids", "list_offsets", "row_pos", "assign", "index"):
        assert torch.equal(getattr(ivf, name), getattr(other, name)), name
    ws, wi = _np(ivf.search_tensors(queries[:32], 10))
    gs, gi = _np(other.search_tensors(queries[:32], 10))
    assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    assert other.search(queries[:3], 5) == ivf.search(queries[:3], 5)


def test_exclude_ids_returns_k_eligible(R):
    ivf, _ = _built(R)
    _, queries = ref.clustered_corpus()
    q = queries[:3]
    first, _ = ivf.search(q, 10)
    excl = [ids[:5] for ids in first]
    again, scores = ivf.search(q, 10, exclude_ids=excl)
    full, _ = ivf.search(q, 15)
    for a, e, f in zip(again, excl, full):
        assert len(a) == 10 and not set(a) & set(e)
        assert a == [i for i in f if i not in e]
    filt, _ = ivf.search(q, 10, filter_ids=first[0][:4])
    assert filt[0] == first[0][:4]


def test_engine_and_refusals(R):
    rows, queries = ref.clustered_corpus()
    eng = R.RetrievalEngine({"index_type": "hip_ivf", "embedding_dim": D, "top_k": 10,
                             "hip_ivf": {"index_factory": f"IVF{NLIST},Flat", "nprobe": 8}})
    assert isinstance(eng.index, R.HipIVFFlatIndex)
    eng.build_index(rows.copy(), _ids(len(rows)))
    ids, scores, metrics = eng.retrieve(queries[:2])
    ivf, _ = _built(R)
    assert (ids, scores) == ivf.search(queries[:2], 10) and metrics["num_results"] == 20
    assert R._INDEX_TYPES["faiss"] is R.HipFlatIPIndex and R._INDEX_TYPES["hip_flat"] is R.HipFlatIPIndex
    with pytest.raises(ValueError, match="HipFlatIPIndex"):
        R.HipIVFFlatIndex(_cfg(metric="l2"))
    with pytest.raises(ValueError):
        R.HipIVFFlatIndex(_cfg(mutable=True))
    with pytest.raises(ValueError):
        R.HipIVFFlatIndex(_cfg(index_factory="HNSW32"))
    assert R.HipIVFFlatIndex({"dimension": D}).nlist == 1024 and R.HipIVFFlatIndex({"dimension": D}).nprobe == 20
    n = ivf.current_size
    ivf.update(rows[:1], ["item_0"])
    assert ivf.remove(["item_0"]) is None and ivf.current_size == n


def test_nprobe_attribute_changes_the_probed_set(R):
    ivf, flat = _built(R)
    _, queries = ref.clustered_corpus()
    _, want = _np(flat.search_tensors(queries, 10))
    try:
        ivf.nprobe = 1
        _, one = _np(ivf.search_tensors(queries, 10))
        assign = ivf.assign.cpu().numpy()
        assert all(len(set(assign[r[r >= 0]])) == 1 for r in one)   # one list per query
        ivf.nprobe = 1000                                            # clamped to nlist: exact
        _, every = _np(ivf.search_tensors(queries, 10))
    finally:
        ivf.nprobe = 8
    assert np.array_equal(every, want)
    assert ref.recall_at_k(one, want) < ref.recall_at_k(every, want) == 1.0


def test_resident_searcher(R, monkeypatch):
    """First (eager), second and third (replayed) call at one shape equal
    search_tensors; nprobe is read at every call; an add in between is picked
    up; RTREC_ONLINE_GRAPH=0 gives the same result."""
    rows, queries = ref.clustered_corpus()
    n0 = len(rows) - 300
    ivf = R.HipIVFFlatIndex(_cfg(storage_dtype="float16"))
    ivf.build(rows[:n0].copy(), _ids(n0))
    s = ivf.online_searcher(8)
    assert isinstance(s, R.OnlineIVFSearcher)

    def check(q, k):
        ws, wi = _np(ivf.search_tensors(q, k))
        gs, gi = s.search(q, k)
        assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))

    for call in range(3):
        check(queries[call * 3:call * 3 + 3], 10)
    check(queries[:1], 100)
    check(queries[1:2], 100)
    ivf.nprobe = 3
    check(queries[:3], 10)
    check(queries[3:6], 10)
    ivf.nprobe = 8
    ivf.add(rows[n0:].copy(), _ids(300, n0))
    check(rows[-3:], 10)
    assert s.search(rows[-1], 1)[1][0, 0] == len(rows) - 1
    # exclusions: the bitmap path, fresh arrays
    ws, wi = _np(ivf.search_tensors(queries[:2], 12))
    gs, gi = s.search(queries[:2], 10, exclude=[wi[0, :2], wi[1, :2]])
    assert np.array_equal(gi, wi[:, 2:])
    monkeypatch.setenv("RTREC_ONLINE_GRAPH", "0")
    check(queries[6:9], 10)
    monkeypatch.delenv("RTREC_ONLINE_GRAPH")
    # through the index: online_max_batch routes small calls to the searcher
    on = R.HipIVFFlatIndex(_cfg(online_max_batch=4))
    on.build(rows.copy(), _ids(len(rows)))
    base, _ = _built(R)
    for _ in range(2):
        assert on.search(queries[:2], 10) == base.search(queries[:2], 10)
    assert isinstance(on._online, R.OnlineIVFSearcher)
