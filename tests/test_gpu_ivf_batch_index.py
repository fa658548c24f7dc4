"""The ``batch_min_queries`` key of HipIVFFlatIndex / HipMutableIVFFlatIndex on
the clustered 8,192 x 32 corpus of tests/_ivf_ref.py with "IVF64,Flat" and
nprobe = 8: calls of that many queries or more take the list-major scan
(kernels.ivf_topk_batch), and an index with the key answers exactly as one
without it — np.array_equal on ids and on the uint32 view of the scores, every
query — through search_tensors, search, RetrievalEngine and the mutable index's
update, add and remove."""
import numpy as np
import pytest
import torch

import _ivf_ref as ref

pytestmark = pytest.mark.gpu

NLIST, D, N = 64, 32, 8192
STORAGES = ["float32", "float16", "bfloat16"]


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


def _corpus():
    return ref.clustered_corpus(n=N, d=D, n_centres=NLIST)


_BUILT = {}


def _pair(R, cls="HipIVFFlatIndex", share=True, **kw):
    """(index without the key, index with batch_min_queries = 16), built from the
    same rows: the build is deterministic, so they hold the same lists."""
    key = (cls,) + tuple(sorted(kw.items()))
    if share and key in _BUILT:
        return _BUILT[key]
    rows, _ = _corpus()
    pair = []
    for extra in ({}, {"batch_min_queries": 16}):
        idx = getattr(R, cls)(_cfg(**kw, **extra))
        idx.build(rows.copy(), _ids(N))
        pair.append(idx)
    for name in ("centroids", "list_offsets", "row_pos", "index"):
        assert torch.equal(getattr(pair[0], name), getattr(pair[1], name)), name
    assert pair[0].batch_min_queries is None and pair[1].batch_min_queries == 16
    if share:
        _BUILT[key] = tuple(pair)
    return tuple(pair)


def _same(a, b, what=""):
    torch.cuda.synchronize()
    (s0, i0), (s1, i1) = [(p[0].cpu().numpy(), p[1].cpu().numpy()) for p in (a, b)]
    assert np.array_equal(i0, i1), what
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), what


def _excl_bits(nq, n, seed=0):
    rng = np.random.default_rng(seed)
    mask = rng.random((nq, n)) < 0.3
    mask[0, :] = True                      # one query excludes everything
    return torch.from_numpy(ref.bitmap_of_excluded(mask).view(np.int32)).cuda()


def _spy(monkeypatch, kernels):
    """Count the calls of kernels.ivf_topk_batch and kernels.ivf_topk."""
    calls = {"batch": 0, "per_query": 0}
    real_b, real_q = kernels.ivf_topk_batch, kernels.ivf_topk

    def batch(*a, **k):
        calls["batch"] += 1
        return real_b(*a, **k)

    def per_query(*a, **k):
        calls["per_query"] += 1
        return real_q(*a, **k)

    monkeypatch.setattr(kernels, "ivf_topk_batch", batch)
    monkeypatch.setattr(kernels, "ivf_topk", per_query)
    return calls


@pytest.mark.parametrize("storage", STORAGES)
def test_search_tensors_identical_with_and_without_the_key(R, storage, monkeypatch):
    plain, keyed = _pair(R, storage_dtype=storage)
    _, queries = _corpus()
    calls = _spy(monkeypatch, R.kernels)
    for nq, batch_calls in ((15, 0), (16, 1), (256, 1)):
        q = queries[:nq]
        for k in (10, 100):
            for bits in (None, _excl_bits(nq, N)):
                calls["batch"] = 0
                got = keyed.search_tensors(q, k, exclude_bits=bits)
                assert calls["batch"] == batch_calls, (nq, calls)
                want = plain.search_tensors(q, k, exclude_bits=bits)
                assert calls["batch"] == batch_calls
                _same(got, want, f"{storage} nq={nq} k={k} bits={bits is not None}")
                if bits is not None:
                    assert (got[1][0] == -1).all()
    assert calls["per_query"] > 0
    # every list probed: the exact search, on both paths
    _same(keyed.search_tensors(queries[:64], 10, nprobe=NLIST), plain.search_tensors(queries[:64], 10, nprobe=NLIST))


def test_search_with_exclude_ids_and_filter_ids(R):
    plain, keyed = _pair(R)
    _, queries = _corpus()
    q = queries[:40]
    first_ids, _ = plain.search(q, 10)
    exclude = [ids[:3] for ids in first_ids]                       # per query: its own top three
    allow = sorted({i for ids in first_ids for i in ids[::2]} | set(_ids(50)))
    for kw in ({}, {"exclude_ids": exclude}, {"exclude_ids": _ids(200)}, {"filter_ids": allow},
               {"filter_ids": allow, "exclude_ids": exclude}):
        want = plain.search(q, 10, **kw)
        got = keyed.search(q, 10, **kw)
        assert got == want, kw
    got_ids, _ = keyed.search(q, 10, exclude_ids=exclude)
    assert all(not set(g) & set(e) for g, e in zip(got_ids, exclude))


def test_engine_passes_the_key_through(R, monkeypatch):
    rows, queries = _corpus()
    engines = []
    for extra in ({}, {"batch_min_queries": 16}):
        e = R.RetrievalEngine({"index_type": "hip_ivf", "embedding_dim": D,
                               "hip_ivf": {"index_factory": f"IVF{NLIST},Flat", "nprobe": 8, **extra}})
        e.build_index(rows.copy(), _ids(N))
        engines.append(e)
    assert engines[0].index.batch_min_queries is None and engines[1].index.batch_min_queries == 16
    calls = _spy(monkeypatch, R.kernels)
    want = engines[0].retrieve(queries[:32], k=10, use_cache=False)
    assert calls["batch"] == 0
    got = engines[1].retrieve(queries[:32], k=10, use_cache=False)
    assert calls["batch"] == 1
    assert got[0] == want[0] and got[1] == want[1]
    got = engines[1].retrieve(queries[:32], k=10, exclude_ids=_ids(100))
    want = engines[0].retrieve(queries[:32], k=10, exclude_ids=_ids(100))
    assert got[0] == want[0] and got[1] == want[1]


def test_dispatch(R, monkeypatch):
    """The key above nq: kernels.ivf_topk_batch is never entered; at nq: it is."""
    plain, _ = _pair(R)
    _, queries = _corpus()
    want = plain.search_tensors(queries[:32], 10)
    idx = R.HipIVFFlatIndex(_cfg(batch_min_queries=33))
    rows, _ = _corpus()
    idx.build(rows.copy(), _ids(N))
    called = []

    def boom(*a, **k):
        called.append(1)
        raise AssertionError("the batch scan must not serve this call")

    real = R.kernels.ivf_topk_batch
    monkeypatch.setattr(R.kernels, "ivf_topk_batch", boom)
    _same(idx.search_tensors(queries[:32], 10), want, "below the key: the per-query scan")
    assert not called
    idx.batch_min_queries = 32

    def witness(*a, **k):
        called.append(1)
        return real(*a, **k)

    monkeypatch.setattr(R.kernels, "ivf_topk_batch", witness)
    _same(idx.search_tensors(queries[:32], 10), want, "at the key: the batch scan")
    assert called == [1]
    with pytest.raises(ValueError, match="batch_min_queries"):
        R.HipIVFFlatIndex(_cfg(batch_min_queries=0))


def test_online_max_batch_keeps_the_resident_searcher(R, monkeypatch):
    rows, queries = _corpus()
    idx = R.HipIVFFlatIndex(_cfg(batch_min_queries=1, online_max_batch=8))
    idx.build(rows.copy(), _ids(N))
    plain, _ = _pair(R)
    calls = _spy(monkeypatch, R.kernels)
    assert idx.search(queries[:8], 10) == plain.search(queries[:8], 10)
    assert calls["batch"] == 0 and idx._online is not None       # at or below online_max_batch
    assert idx.search(queries[:9], 10) == plain.search(queries[:9], 10)
    assert calls["batch"] == 1


def test_flat_fallback_ignores_the_key(R, monkeypatch):
    rows, queries = _corpus()
    small = rows[:500].copy()
    a = R.HipIVFFlatIndex(_cfg())
    b = R.HipIVFFlatIndex(_cfg(batch_min_queries=1))
    a.build(small.copy(), _ids(500))
    b.build(small.copy(), _ids(500))
    assert b._flat is not None
    calls = _spy(monkeypatch, R.kernels)
    _same(b.search_tensors(queries[:64], 10), a.search_tensors(queries[:64], 10))
    assert b.search(queries[:20], 10) == a.search(queries[:20], 10)
    assert calls["batch"] == 0


def test_save_load_round_trips_the_key(R, tmp_path):
    _, keyed = _pair(R)
    _, queries = _corpus()
    keyed.save(str(tmp_path / "ivf"))
    again = R.HipIVFFlatIndex({"dimension": D, "index_factory": f"IVF{NLIST},Flat"})
    again.load(str(tmp_path / "ivf"))
    assert again.batch_min_queries == 16
    again.nprobe = keyed.nprobe
    _same(again.search_tensors(queries[:64], 10), keyed.search_tensors(queries[:64], 10))


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_mutable_index_through_update_add_remove(R, storage, monkeypatch):
    """HipMutableIVFFlatIndex: _scan_operands() hands list_len / n_pos to the batch
    scan. Identical results with and without the key before and after an update
    that moves rows between lists, after an add and after a remove."""
    plain, keyed = _pair(R, cls="HipMutableIVFFlatIndex", share=False, storage_dtype=storage)
    rows, queries = _corpus()
    calls = _spy(monkeypatch, R.kernels)
    rng = np.random.default_rng(2)

    def check(what):
        n = keyed.current_size
        for nq in (15, 64):
            for bits in (None, _excl_bits(nq, n, seed=3)):
                before = calls["batch"]
                got = keyed.search_tensors(queries[:nq], 100, exclude_bits=bits)
                assert calls["batch"] == before + (nq >= 16)
                _same(got, plain.search_tensors(queries[:nq], 100, exclude_bits=bits), f"{what} nq={nq}")
        assert keyed.search(queries[:20], 10, exclude_ids=_ids(64)) == plain.search(queries[:20], 10,
                                                                                   exclude_ids=_ids(64))

    check("built")
    known = rng.choice(N, 60, replace=False)
    moved = (rows[rng.integers(0, N, 60)] + 0.02 * rng.standard_normal((60, D))).astype(np.float32)
    before = keyed.assign[:N].clone()
    for idx in (plain, keyed):
        idx.update(moved.copy(), [f"item_{p}" for p in known])
    assert int((keyed.assign[:N] != before).sum()) >= 5, "the update must move rows between lists"
    check("after update")
    new = (rows[rng.integers(0, N, 50)] + 0.02 * rng.standard_normal((50, D))).astype(np.float32)
    for idx in (plain, keyed):
        idx.add(new.copy(), _ids(50, start=20000))
    assert keyed.current_size == N + 50
    check("after add")
    out = [f"item_{p}" for p in rng.choice(N, 40, replace=False)]
    for idx in (plain, keyed):
        assert idx.remove(out) == 40
    check("after remove")
