"""HipMutableIVFFlatIndex: update / add / remove in place on "IVF16,Flat" over the
clustered 2,048 x 32 corpus of tests/_ivf_ref.py. The item-level model of
tests/_ivf_mutate_ref.py says which row and which list every position holds
after each call; searches are then checked exactly (score bits and positions)
against the C oracle restricted to the probed lists over the model's rows in
position order, and at nprobe = nlist against a HipFlatIPIndex built on the same
live items, by item id."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _ivf_mutate_ref as mref
import _ivf_ref as ref

pytestmark = pytest.mark.gpu

NLIST, D, N, K_TOP = 16, 32, 2048, 10
F, USERS = 10, 16


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
    cfg = {"dimension": D, "index_factory": f"IVF{NLIST},Flat", "metric": "cosine", "nprobe": 4}
    cfg.update(kw)
    return cfg


def _corpus(metric="cosine"):
    rows, queries = ref.clustered_corpus(n=N, d=D, n_centres=NLIST)
    scale = 1.0 if metric == "cosine" else 1.5      # inner product: rows and queries that are not unit vectors
    return rows * scale, queries[:8] * (1.0 if metric == "cosine" else 3.0)


def _built(R, **kw):
    rows, _ = _corpus(kw.get("metric", "cosine"))
    idx = R.HipMutableIVFFlatIndex(_cfg(**kw))
    idx.build(rows.copy(), _ids(N))
    return idx


def _bits(t):
    if t.dtype == torch.float32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), 1


class _Model(mref.IndexModel):
    """The item model with rows as the index prepares and stores them: a payload of
    (raw embedding, stored row), the list by fp64 argmax over the index's centroids."""

    def __init__(self, idx, raw, ids):
        self.idx = idx
        rows, lists = self._prepared(raw)
        super().__init__(ids, rows, lists)

    def _prepared(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        p = self.idx._prepare(raw)
        stored = p.to(self.idx.storage_dtype).cpu()
        lists = ref.assign(p.cpu().numpy(), self.idx.centroids.cpu().numpy())
        return [(raw[i], stored[i]) for i in range(len(raw))], lists

    def update(self, ids, raw):
        super().update(list(ids), *self._prepared(raw))

    def add(self, ids, raw, lists=None):
        if lists is None:
            raw, lists = self._prepared(raw)
        super().add(list(ids), raw, lists)

    def stored(self):
        return torch.stack([s for _, s in self.rows])

    def raw(self):
        return np.stack([r for r, _ in self.rows])


def _check(R, idx, model, queries, flat=True):
    """The index against the model: the id maps, the device state's invariants, and
    the searches at nprobe = 4 and nprobe = nlist."""
    n = len(model.ids)
    assert idx.current_size == n
    assert idx.id_map == dict(enumerate(model.ids))
    assert idx.reverse_id_map == model.where()
    assert idx._ids[:n] == model.ids
    state = type("S", (), {name: getattr(idx, name).cpu().numpy() for name in ("row_pos", "pos_slot", "assign",
                                                                             "list_len")})
    offsets = idx.list_offsets.cpu().numpy()
    mref.check_invariants(state, offsets)
    assert np.array_equal(state.assign[:n], np.asarray(model.lists)) and (state.assign[n:] == -1).all()
    assert idx.capacity == offsets[-1] == len(idx.index) and idx.max_list_rows == np.diff(offsets).max()
    assert np.array_equal(idx.vectors(), model.stored().float().numpy())
    q32 = idx._prepare(queries)
    qs = q32.to(idx.storage_dtype).cpu()
    qa, code = _bits(qs)
    xa = _bits(model.stored())[0]
    for nprobe in (4, NLIST):
        probes = ref.coarse_probes(q32.cpu().numpy(), idx.centroids.cpu().numpy(), nprobe)
        rs, ri = ref.probed_lists_search(qa, xa, model.lists, probes, K_TOP, dtype_code=code)
        gs, gi = idx.search_tensors(queries, K_TOP, nprobe=nprobe)
        gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
        assert np.array_equal(gi, ri), (nprobe, gi[:2], ri[:2])
        assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), nprobe
    if flat:
        exact = R.HipFlatIPIndex({"dimension": D, "metric": idx.metric, "online_max_batch": 8,
                                  "storage_dtype": idx.config.get("storage_dtype", "float32")})
        exact.build(model.raw(), list(model.ids))
        idx.nprobe = NLIST
        try:
            assert idx.search(queries, K_TOP) == exact.search(queries, K_TOP)
        finally:
            idx.nprobe = 4


def _moved_rows(rng, base, n, m):
    """m embeddings near OTHER rows of the corpus: far enough to change list."""
    return base[rng.integers(0, n, m)] + 0.02 * rng.standard_normal((m, D)).astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_update_add_remove_against_the_model(R, metric, storage):
    idx = _built(R, metric=metric, storage_dtype=storage)
    rows, queries = _corpus(metric)
    model = _Model(idx, rows, _ids(N))
    assert idx.mutable and isinstance(idx, R.HipIVFFlatIndex)
    _check(R, idx, model, queries)
    rng = np.random.default_rng(1)
    gen = idx._generation

    # update: 20 rows nudged, 20 moved next to other rows, one id twice (the last wins), 3 unknown ids
    known = rng.choice(N, 40, replace=False)
    emb = np.concatenate([rows[known[:20]] + 0.01 * rng.standard_normal((20, D)).astype(np.float32),
                          _moved_rows(rng, rows, N, 20), _moved_rows(rng, rows, N, 4)]).astype(np.float32)
    ids = [f"item_{p}" for p in known] + [f"item_{known[3]}", "fresh_0", "fresh_1", "fresh_0"]
    before = list(model.lists)
    in_place_only = len(ids) - 3
    idx.update(emb[:in_place_only].copy(), ids[:in_place_only])
    assert idx._generation == gen                     # known ids only: nothing a captured graph holds changed
    model.update(ids[:in_place_only], emb[:in_place_only])
    assert sum(a != b for a, b in zip(before, model.lists)) >= 5, "the update must move rows between lists"
    _check(R, idx, model, queries, flat=False)
    idx.update(emb.copy(), ids)                       # the same again plus the unknown ids: appended in call order
    model.update(ids, emb)
    assert model.ids[-2:] == ["fresh_0", "fresh_1"] and idx._generation > gen
    _check(R, idx, model, queries)

    # add: 50 rows, one under an id that is already stored (stored again; reverse_id_map names the last row)
    new = _moved_rows(rng, rows, N, 50).astype(np.float32)
    new_ids = _ids(49, start=5000) + ["item_7"]
    gen = idx._generation
    idx.add(new.copy(), new_ids)
    model.add(new_ids, new)
    assert idx._generation > gen and idx.reverse_id_map["item_7"] == len(model.ids) - 1
    _check(R, idx, model, queries, flat=False)        # two rows under one id: no Flat index by id

    # remove: 30 ids, the twice-stored one among them (both rows go), an unknown id ignored
    out = [f"item_{p}" for p in rng.choice(np.arange(8, N), 28, replace=False)] + ["item_7", "fresh_1", "nobody"]
    gen = idx._generation
    n_removed, moves = model.remove(out)
    assert idx.remove(out) == n_removed == 31 and idx._generation > gen and moves
    assert idx.remove(["nobody"]) == 0
    _check(R, idx, model, queries)


def test_position_tie_rule_after_remove(R):
    """Two items with one vector tie on score and resolve by position. Stored at the
    last two positions, the first one wins; after a remove that renumbers the
    last position into a low hole, the other one does — the documented rule, not
    the order of a rebuilt index."""
    idx = _built(R)
    rows, queries = _corpus()
    v = queries[:1]
    idx.add(np.concatenate([v, v]), ["twin_a", "twin_b"])
    idx.nprobe = NLIST
    ids, scores = idx.search(v, 2)
    assert ids == [["twin_a", "twin_b"]] and scores[0][0] == scores[0][1]
    assert idx.remove(["item_5"]) == 1                    # n' = N + 1: position N + 1 (twin_b) takes position 5
    assert idx.reverse_id_map["twin_b"] == 5 and idx.reverse_id_map["twin_a"] == N
    ids, scores = idx.search(v, 2)
    assert ids == [["twin_b", "twin_a"]] and scores[0][0] == scores[0][1]


def test_overflow_regroups(R):
    """One spare row per list: an update that moves six rows into one list cannot be
    applied in place; the index regroups once with fresh slack and is right."""
    idx = _built(R, list_slack=0.0, min_slack_rows=1)
    rows, queries = _corpus()
    model = _Model(idx, rows, _ids(N))
    lens = np.bincount(model.lists, minlength=NLIST)
    off = idx.list_offsets.cpu().numpy()
    assert np.array_equal(np.diff(off), mref.capacities(lens, 0.0, 1)) and idx.capacity == N + NLIST
    target = int(np.argmax(lens))
    anchor = idx.centroids[target].cpu().numpy()                 # rows next to a centroid are assigned to it
    movers = [p for p, l in enumerate(model.lists) if l != target][:6]
    emb = (anchor + 0.01 * np.random.default_rng(2).standard_normal((6, D))).astype(np.float32)
    gen = idx._generation
    idx.update(emb.copy(), [f"item_{p}" for p in movers])
    model.update([f"item_{p}" for p in movers], emb)
    assert [model.lists[p] for p in movers] == [target] * 6
    assert idx._generation > gen                              # regrouped: pointers and capacities changed
    assert np.array_equal(np.diff(idx.list_offsets.cpu().numpy()),
                          mref.capacities(np.bincount(model.lists, minlength=NLIST), 0.0, 1))
    _check(R, idx, model, queries)
    # add past the total capacity: a regroup too
    new = _moved_rows(np.random.default_rng(3), rows, N, 40).astype(np.float32)
    idx.add(new.copy(), _ids(40, start=9000))
    model.add(_ids(40, start=9000), new)
    _check(R, idx, model, queries)


def test_defaults_and_capacity_rule(R):
    idx = _built(R)
    assert idx.list_slack == 0.25 and idx.min_slack_rows == 32
    lens = idx.list_len.cpu().numpy()
    assert lens.sum() == N
    assert np.array_equal(np.diff(idx.list_offsets.cpu().numpy()), mref.capacities(lens))
    with pytest.raises(ValueError, match="HipMutableIVFFlatIndex"):
        R.HipIVFFlatIndex(_cfg(mutable=True))
    with pytest.raises(ValueError):
        R.HipMutableIVFFlatIndex(_cfg(list_slack=-1))


def test_save_load_round_trip(R, tmp_path):
    idx = _built(R, storage_dtype="float16")
    rows, queries = _corpus()
    rng = np.random.default_rng(4)
    idx.update(_moved_rows(rng, rows, N, 30).astype(np.float32), [f"item_{p}" for p in rng.choice(N, 30, False)])
    idx.add(_moved_rows(rng, rows, N, 10).astype(np.float32), _ids(10, start=7000))
    assert idx.remove(_ids(25, start=100)) == 25
    idx.save(str(tmp_path / "ivf"))
    vecs, _ = R.read_flat_index(tmp_path / "ivf.faiss")
    assert vecs.shape == (N + 10 - 25, D)                        # live rows only, in position order
    assert np.array_equal(vecs, idx.vectors())
    back = R.HipMutableIVFFlatIndex(_cfg(storage_dtype="float16"))
    back.load(str(tmp_path / "ivf"))
    assert back.current_size == idx.current_size and back.id_map == idx.id_map and back.mutable
    for nprobe in (4, NLIST):
        a, b = idx.search_tensors(queries, K_TOP, nprobe=nprobe), back.search_tensors(queries, K_TOP, nprobe=nprobe)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert back.search(queries, 5) == idx.search(queries, 5)
    assert back.remove(["item_0"]) == 1                          # a loaded index mutates


def test_engine(R):
    rows, queries = _corpus()
    engine = R.RetrievalEngine({"index_type": "hip_ivf_mutable", "embedding_dim": D,
                                "hip_ivf_mutable": {"index_factory": f"IVF{NLIST},Flat", "nprobe": NLIST}})
    assert isinstance(engine.index, R.HipMutableIVFFlatIndex)
    engine.build_index(rows.copy(), _ids(N))
    q = queries[:2]
    engine.update_index(np.concatenate([q, q[:1]]), ["item_3", "item_4", "brand_new"], upsert=True)
    assert engine.index.current_size == N + 1 and len(engine.index.reverse_id_map) == N + 1   # one row per id
    ids, scores, _ = engine.retrieve(q, k=3, use_cache=False)
    assert set(ids[0][:2]) == {"item_3", "brand_new"} and ids[1][0] == "item_4"
    assert engine.remove_items(["item_3", "item_4", "nobody"]) == 2
    ids, _, _ = engine.retrieve(q, k=3, use_cache=False)
    assert ids[0][0] == "brand_new" and "item_3" not in ids[0] and "item_4" not in ids[1]
    assert engine.get_metrics()["index_size"] == N - 1


def test_flat_fallback_mutates(R):
    rows, queries = _corpus()
    idx = R.HipMutableIVFFlatIndex(_cfg())
    idx.build(rows[:500].copy(), _ids(500))
    assert isinstance(idx._flat, R.HipFlatIPIndex) and idx._flat.mutable and idx.centroids is None
    q = queries[:1]
    idx.update(np.concatenate([q, q]), ["item_9", "extra"])
    assert idx.current_size == 501 and set(idx.search(q, 2)[0][0]) == {"item_9", "extra"}
    assert idx.remove(["item_9", "nobody"]) == 1 and idx.current_size == 500
    assert idx.search(q, 1)[0] == [["extra"]]
    idx.add(q.copy(), ["again"])
    assert idx.current_size == 501 and set(idx.search(q, 2)[0][0]) == {"extra", "again"}


def test_emptied_index_returns_empty_lists(R):
    idx = _built(R)
    _, queries = _corpus()
    assert idx.remove(_ids(N)) == N and idx.current_size == 0
    assert idx.search(queries[:3], 5) == ([[], [], []], [[], [], []])
    s, p = idx.search_tensors(queries[:3], 5)
    assert (p.cpu().numpy() == -1).all()
    assert not idx.id_map and not idx.reverse_id_map
    idx.add(queries[:2].copy(), ["a", "b"])                       # and fills again
    assert idx.search(queries[:1], 1)[0] == [["a"]] and idx.current_size == 2


def test_resident_searcher_keeps_its_graphs_through_an_update(R):
    idx = _built(R, online_max_batch=4)
    rows, queries = _corpus()
    q = queries[:2]

    def unresident(**kw):
        idx.online_max_batch = 0
        try:
            return idx.search(q, K_TOP, **kw)
        finally:
            idx.online_max_batch = 4

    first = idx.search(q, K_TOP)
    assert idx.search(q, K_TOP) == first == unresident()          # eager, then the captured graph
    searcher = idx._online
    assert isinstance(searcher, R.OnlineIVFSearcher)
    graphs = dict(searcher._graphs)
    gen = idx._generation
    assert graphs and "item_1500" not in first[0][0]
    # in place: item_1500 becomes query 0's direction — another list, the best row
    idx.update(q[:1].copy(), ["item_1500"])
    assert idx._generation == gen and idx._online is searcher
    got = idx.search(q, K_TOP)
    assert dict(searcher._graphs) == graphs and all(searcher._graphs[k] is g for k, g in graphs.items())
    assert got[0][0][0] == "item_1500" and got == unresident() and got != first
    # add and remove bump the generation; the searcher recaptures and answers right
    idx.add(q[1:2].copy(), ["late"])
    assert idx._generation > gen
    got = idx.search(q, K_TOP)
    assert got[0][1][0] == "late" and got == unresident() and idx.search(q, K_TOP) == got
    gen = idx._generation
    assert idx.remove(["item_1500", "item_2"]) == 2 and idx._generation > gen
    got = idx.search(q, K_TOP)
    assert "item_1500" not in got[0][0] and got == unresident() and idx.search(q, K_TOP) == got
    excl = [[], ["late"]]
    got = idx.search(q, K_TOP, exclude_ids=excl)                  # the scan reads the lists: rt_ivf_topk_lists_lens
    assert got == unresident(exclude_ids=excl) and "late" not in got[0][1] and len(got[0][1]) == K_TOP


def _tower_model(seed=0):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    torch.manual_seed(seed)
    user = UserTower(F, embedding_dim=D, hidden_layers=[64, 32], dropout_rate=0.2)
    item = ItemTower(6, embedding_dim=D, hidden_layers=[16], use_content_embedding=False)
    with torch.no_grad():
        for mod in user.mlp:
            if isinstance(mod, nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
    return TwoTowerModel(user, item).to("cuda")


def test_recommender_seen_items_follow_a_renumbering(R):
    """A seen item that remove renumbers stays excluded for its user (the
    recommender remaps its seen lists by generation), and a removed item is never
    returned."""
    from rtrec_amd import serving as S
    idx = _built(R)
    idx.nprobe = NLIST
    feats = np.random.default_rng(42).standard_normal((USERS, F)).astype(np.float32)
    rec = S.OnlineRecommender(_tower_model(), idx, user_table=torch.from_numpy(feats.copy()).cuda())
    uid = np.array([3])
    e = rec.embed(user_ids=uid).copy()
    last = f"item_{N - 1}"
    idx.update(e.copy(), [last])                                  # the last position: the user's best item
    base = rec.recommend(user_ids=uid, k=8)
    assert base == idx.search(e, 8) and base[0][0][0] == last
    victim, hole = base[0][0][1], "item_11"                       # the runner-up is withdrawn, with a low position
    assert hole not in base[0][0]
    seen = {3: [last, base[0][0][2]]}
    rec.set_seen(seen)
    got = rec.recommend(user_ids=uid, k=8, exclude_seen=True)
    assert got == idx.search(e, 8, exclude_ids=[seen[3]]) and last not in got[0][0]
    gone = (11, idx.reverse_id_map[victim])
    assert idx.remove([hole, victim]) == 2
    assert idx.reverse_id_map[last] in gone                       # renumbered into one of the two holes
    got = rec.recommend(user_ids=uid, k=8, exclude_seen=True)
    assert got == idx.search(e, 8, exclude_ids=[seen[3]])
    assert last not in got[0][0] and victim not in got[0][0] and seen[3][1] not in got[0][0]
    assert len(got[0][0]) == 8
    plain = rec.recommend(user_ids=uid, k=8)
    assert plain[0][0][0] == last and victim not in plain[0][0]
