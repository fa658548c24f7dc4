"""Category filters through the index classes, the resident searchers, the
recommender and the engine: every route returns the same lists and the
reference's ids (the filter as the exclusion bitmap of the ineligible items,
_tag_filter_ref), graphs are shared by all mask values, tags change in place
and follow the index's own renumbering, and survive save / load."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _ivf_ref as ref
import _tag_filter_ref as tref
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

D, NLIST, F, USERS = 32, 64, 12, 64
VOCAB = [f"c{j}" for j in range(64)]
KINDS = ["flat", "ivf", "ivf_mutable"]


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native, serving
    native.lib()
    return serving


def _ids(n, start=0):
    return [f"item_{i}" for i in range(start, start + n)]


def _make(S, kind, **kw):
    cfg = {"dimension": D, "metric": "inner_product", "categories": VOCAB, "online_max_batch": 8}
    if kind == "flat":
        cfg["mutable"] = True
        cls = S.HipFlatIPIndex
    else:
        cfg.update(index_factory=f"IVF{NLIST},Flat", nprobe=8)
        from rtrec_amd.serving.retrieval import HipMutableIVFFlatIndex
        cls = S.HipIVFFlatIndex if kind == "ivf" else HipMutableIVFFlatIndex
    cfg.update(kw)
    return cls(cfg)


def _built(S, kind, n=None, **kw):
    rows, _ = ref.clustered_corpus()
    n = len(rows) if n is None else n
    index = _make(S, kind, **kw)
    index.build(rows[:n].copy(), _ids(n), item_categories=tref.fixture_tags(n))
    return index


def _names(nq):
    """The fixture's masks as names: per query one list to filter on, one to exclude."""
    return [[f"c{q % 7}"] for q in range(nq)], [[f"c{7 + q % 5}"] for q in range(nq)]


def _reference_ids(index, queries, k, excluded=None):
    """Ids of the filtered search over what the index scans: the corpus (Flat) or
    the probed lists under the index's own centroids and assignment (IVF)."""
    n, nq = index.current_size, len(queries)
    rows = np.ascontiguousarray(index.vectors())
    any_of, none_of = tref.fixture_masks(nq)
    bits = tref.filter_bits(index.item_tags(), any_of, none_of)
    if excluded is not None:
        m = np.zeros((nq, n), bool)
        for q, e in enumerate(excluded):
            m[q, [index.reverse_id_map[i] for i in e]] = True
        bits = bits | ref.bitmap_of_excluded(m)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if getattr(index, "centroids", None) is None:
        pos = orc.flat_ip_search(q, rows, k, exclude_bits=bits, nthreads=16)[1]
    else:
        probes = ref.coarse_probes(q, index.centroids.cpu().numpy(), index._n_probe())
        pos = ref.probed_lists_search(q, rows, index._live_assign().cpu().numpy(), probes, k, exclude_bits=bits)[1]
    return [[index.id_map[int(p)] for p in row if p >= 0] for row in pos]


# ---- routing -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_route_returns_the_reference(S, kind):
    index = _built(S, kind)
    queries = ref.clustered_corpus()[1][:16].copy()
    k = 20
    fc, xc = _names(16)
    want = _reference_ids(index, queries, k)
    assert all(len(r) >= 10 for r in want)
    # the bitmap route: more queries than online_max_batch
    via_bitmap = index.search(queries, k, filter_categories=fc, exclude_categories=xc)
    assert via_bitmap[0] == want
    # the resident route: the masks of queries 8.. belong to the second call
    assert index._online is None
    a = index.search(queries[:8], k, filter_categories=fc[:8], exclude_categories=xc[:8])
    b = index.search(queries[8:], k, filter_categories=fc[8:], exclude_categories=xc[8:])
    assert index._online is not None and len(index._online._graphs) == 1
    assert (a[0] + b[0], a[1] + b[1]) == via_bitmap
    # with exclude_ids on top, on both routes
    excluded = [row[:3] for row in want]
    want_x = _reference_ids(index, queries, k, excluded)
    assert index.search(queries, k, exclude_ids=excluded, filter_categories=fc, exclude_categories=xc)[0] == want_x
    assert index.search(queries[:8], k, exclude_ids=excluded[:8], filter_categories=fc[:8],
                        exclude_categories=xc[:8])[0] == want_x[:8]
    if kind != "flat":   # the list-major batch scan
        index.batch_min_queries = 4
        assert index.search(queries, k, filter_categories=fc, exclude_categories=xc) == via_bitmap
        assert index.search(queries, k, exclude_ids=excluded, filter_categories=fc, exclude_categories=xc)[0] == want_x
        index.batch_min_queries = None
    # one list of names for all queries; search_tensors takes masks
    one = index.search(queries, k, filter_categories=["c2", "c3"], exclude_categories="c8")
    s, p = index.search_tensors(queries, k, tag_filter=(np.full(16, (1 << 2) | (1 << 3), np.uint64),
                                                        np.full(16, 1 << 8, np.int64)))
    assert one[0] == [[index.id_map[int(i)] for i in row if i >= 0] for row in p.cpu().numpy()]
    tags = index.item_tags()
    for row in p.cpu().numpy():
        assert all(int(tags[i]) & 0b1100 and not int(tags[i]) & (1 << 8) for i in row if i >= 0)


def test_small_ivf_corpus_forwards_to_the_flat_fallback(S):
    index = _built(S, "ivf", n=900)
    assert index._flat is not None and index._flat.categories == VOCAB
    queries = ref.clustered_corpus()[1][:8].copy()
    fc, xc = _names(8)
    got = index.search(queries, 10, filter_categories=fc, exclude_categories=xc)
    assert got[0] == _reference_ids(index, queries, 10)
    assert index.search(np.concatenate([queries, queries]), 10, filter_categories=fc + fc,
                        exclude_categories=xc + xc)[0] == got[0] + got[0]


# ---- graphs, in-place tag changes ----------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_masks_and_tags_change_under_one_graph(S, kind):
    index = _built(S, kind)
    queries = ref.clustered_corpus()[1][:4].copy()
    k = 10
    seen = []
    for j in range(4):   # masks changing between calls
        got = index.search(queries, k, filter_categories=[f"c{j}"], exclude_categories=[f"c{8 + j % 3}"])
        assert all(len(r) == k for r in got[0])
        seen.append(got[0])
    searcher = index._online
    assert len(searcher._graphs) == 1 and len({str(s) for s in seen}) == 4
    assert index.search(queries, k)[0] != seen[0] and len(searcher._graphs) == 2   # unfiltered: its own graph
    gen = index._generation
    # set_item_categories: the best item of every query leaves the filter, the next result lacks it
    best = sorted({row[0] for row in seen[0]})
    index.set_item_categories(best, [["c5"]] * len(best))
    after = index.search(queries, k, filter_categories=["c0"], exclude_categories=["c8"])
    assert not set(best) & {i for row in after[0] for i in row}
    for old, new in zip(seen[0], after[0]):
        left = [i for i in old if i not in best]
        assert new[:len(left)] == left
    assert index._generation == gen and index._online is searcher and len(searcher._graphs) == 2
    if kind != "ivf":   # update with new tags: in place too (the IVF index without slack only warns)
        rows = ref.clustered_corpus()[0]
        pos = [index.reverse_id_map[i] for i in best]
        index.update(rows[pos].copy(), best, item_categories=[["c0", "c9"]] * len(best))
        again = index.search(queries, k, filter_categories=["c0"], exclude_categories=["c8"])
        assert again == (seen[0], again[1])
        index.update(rows[pos].copy(), best)   # None keeps the tags
        assert index.search(queries, k, filter_categories=["c0"], exclude_categories=["c8"]) == again
        assert index._generation == gen and len(searcher._graphs) == 2


# ---- renumbering ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "ivf_mutable"])
def test_tags_follow_add_and_remove(S, kind):
    rows, queries = ref.clustered_corpus()
    n0, n = 6000, 8192
    tags = tref.fixture_tags(n)
    kw = {} if kind == "flat" else {"nprobe": NLIST}   # every list: results do not depend on the training
    index = _make(S, kind, **kw)
    index.build(rows[:n0].copy(), _ids(n0), item_categories=tags[:n0])
    index.add(rows[n0:].copy(), _ids(n - n0, n0), item_categories=tags[n0:])
    gone = np.unique(np.random.default_rng(5).integers(0, n, 700))
    assert index.remove([f"item_{i}" for i in gone]) == len(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    fresh = _make(S, kind, **kw)
    fresh.build(rows[keep].copy(), [f"item_{i}" for i in keep], item_categories=tags[keep])
    by_id = dict(zip((f"item_{i}" for i in range(n)), tags.tolist()))
    assert [by_id[index.id_map[p]] for p in range(index.current_size)] == index.item_tags().tolist()
    fc, xc = _names(16)
    for q in (queries[:8].copy(), queries[:16].copy()):   # resident and bitmap route
        nq = len(q)
        got = index.search(q, 20, filter_categories=fc[:nq], exclude_categories=xc[:nq])
        want = fresh.search(q, 20, filter_categories=fc[:nq], exclude_categories=xc[:nq])
        assert got == want and all(len(r) == 20 for r in got[0])


# ---- persistence ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_save_load_round_trip(S, kind, tmp_path):
    index = _built(S, kind)
    queries = ref.clustered_corpus()[1][:16].copy()
    fc, xc = _names(16)
    want8 = index.search(queries[:8], 20, filter_categories=fc[:8], exclude_categories=xc[:8])
    want16 = index.search(queries, 20, filter_categories=fc, exclude_categories=xc)
    index.save(str(tmp_path / "idx"))
    assert (tmp_path / "idx.tags.npz").exists()
    loaded = _make(S, kind, categories=None)   # the vocabulary comes from the file
    loaded.load(str(tmp_path / "idx"))
    assert loaded.categories == VOCAB and np.array_equal(loaded.item_tags(), index.item_tags())
    assert loaded.search(queries[:8], 20, filter_categories=fc[:8], exclude_categories=xc[:8]) == want8
    assert loaded.search(queries, 20, filter_categories=fc, exclude_categories=xc) == want16


# ---- recommender, engine ----------------------------------------------------------------
def _model(dim=D):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    torch.manual_seed(0)
    user = UserTower(F, embedding_dim=dim, hidden_layers=[64, 32], dropout_rate=0.2)
    item = ItemTower(6, embedding_dim=dim, hidden_layers=[16], use_content_embedding=False)
    with torch.no_grad():
        for mod in user.mlp:
            if isinstance(mod, nn.Linear):
                mod.bias.uniform_(-0.1, 0.1)
    return TwoTowerModel(user, item).to("cuda")


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_recommend_with_categories_and_seen(S, kind):
    index = _built(S, kind, metric="cosine")
    feats = np.random.default_rng(42).standard_normal((USERS, F)).astype(np.float32)
    rec = S.OnlineRecommender(_model(), index, user_table=torch.from_numpy(feats.copy()).cuda())
    uid = np.array([5, 9, 63, 0])
    e = rec.embed(user_ids=uid).copy()
    fc, xc = _names(4)
    base = index.search(e, 20, filter_categories=fc, exclude_categories=xc)[0]
    histories = {int(u): base[q][:3 + q] for q, u in enumerate(uid)}
    rec.set_seen(histories)
    seen = [histories[int(u)] for u in uid]
    for items in (None, [row[5:8] for row in base]):
        excl = seen if items is None else [s + i for s, i in zip(seen, items)]
        got = rec.recommend(user_ids=uid, k=20, exclude_seen=True, exclude_items=items, filter_categories=fc,
                            exclude_categories=xc)
        assert got == index.search(e, 20, exclude_ids=excl, filter_categories=fc, exclude_categories=xc)
        assert all(len(r) >= 5 for r in got[0])
        assert not any(set(r) & set(x) for r, x in zip(got[0], excl))
    n_graphs = len(rec._graphs)
    got = rec.recommend(user_ids=uid, k=20, exclude_seen=True, exclude_items=[row[5:8] for row in base],
                        filter_categories=[["c1"]] * 4)   # other masks: the same graph
    assert len(rec._graphs) == n_graphs
    assert got == index.search(e, 20, exclude_ids=[s + r[5:8] for s, r in zip(seen, base)],
                               filter_categories=[["c1"]] * 4)
    # features instead of ids, without exclusions
    assert rec.recommend(feats[:2], k=10, filter_categories=["c3"]) == \
        index.search(rec.embed(feats[:2]).copy(), 10, filter_categories=["c3"])


def test_engine_bypasses_the_cache_for_a_filtered_call(S):
    rows, queries = ref.clustered_corpus()
    engine = S.RetrievalEngine({"index_type": "hip_flat", "embedding_dim": D, "top_k": 10,
                                "hip_flat": {"metric": "inner_product", "categories": VOCAB, "online_max_batch": 8}})
    engine.build_index(rows.copy(), _ids(len(rows)), item_categories=tref.fixture_tags(len(rows)))
    q = queries[:2].copy()
    plain = engine.retrieve(q)
    assert len(engine.cache) == 1 and engine.retrieve(q)[2]["cache_hit"]
    ids, scores, m = engine.retrieve(q, filter_categories=["c1"], exclude_categories=["c9"])
    assert not m["cache_hit"] and len(engine.cache) == 1 and engine.cache_hits == 1
    assert (ids, scores) == engine.index.search(q, 10, filter_categories=["c1"], exclude_categories=["c9"])
    assert ids != plain[0]
    assert not engine.retrieve(q, filter_categories=["c1"])[2]["cache_hit"] and engine.cache_hits == 1


# ---- refusals ------------------------------------------------------------------------
def test_refusals(S):
    index = _built(S, "flat", n=2000)
    q = ref.clustered_corpus()[1][:2].copy()
    with pytest.raises(ValueError, match="unknown category"):
        index.search(q, 5, filter_categories=["horror"])
    with pytest.raises(ValueError, match="unknown category"):
        index.search(q, 5, exclude_categories=[["c1"], ["nope"]])
    with pytest.raises(ValueError, match="unknown ids"):
        index.set_item_categories(["item_1", "zzz"], [["c1"], ["c2"]])
    with pytest.raises(ValueError, match="2 entries for 1 items"):
        index.add(q[:1], ["new"], item_categories=[["c1"], ["c2"]])
    rows = ref.clustered_corpus()[0]
    for kind in KINDS:
        plain = _make(S, kind, categories=None)
        with pytest.raises(ValueError, match="'categories'"):
            plain.build(rows[:2000].copy(), _ids(2000), item_categories=tref.fixture_tags(2000))
        plain.build(rows[:2000].copy(), _ids(2000))
        for kw in ({"filter_categories": ["c1"]}, {"exclude_categories": ["c1"]}):
            with pytest.raises(ValueError, match="'categories'"):
                plain.search(q, 5, **kw)
        with pytest.raises(ValueError, match="'categories'"):
            plain.search_tensors(q, 5, tag_filter=(np.ones(2, np.uint64), None))
        with pytest.raises(ValueError, match="'categories'"):
            plain.set_item_categories(["item_1"], [["c1"]])
        with pytest.raises(ValueError, match="'categories'"):
            plain.add(q[:1], ["new"], item_categories=[["c1"]])
        assert plain.search(q, 5)[0] == plain.search(q, 5, filter_categories=None)[0]
