"""``HipFlatIPIndex`` with ``mutable: True``: after every step of build -> remove
-> update (upsert) -> add -> remove the index is indistinguishable from a fresh
one built on the surviving raw rows and ids in order — the same lists (ids
equal, scores equal as floats: both paths are deterministic and per-row, so
there is no tolerance), the same stored bits, consistent id maps — and resident
searchers keep their captured graphs over an in-place update and drop them on a
removal."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = 5000, 32
PLANT = (100, 2500, 4000)        # identical rows at i < j < l; i leaves in the first removal: j must then win over l
NQ, KS = (1, 8, 40), (10, 128)

CONFIGS = [(m, s, o) for m in ("cosine", "inner_product") for s in ("float32", "float16", "bfloat16") for o in (8, 0)]
CONFIGS.append(("l2", "float32", 0))


def _dyadic(rng, n, d, lo=-64, hi=64):
    return (rng.integers(lo, hi + 1, size=(n, d)) / 64.0).astype(np.float32)


def _id(n):
    return f"item_{n}"


@pytest.fixture(autouse=True)
def _collect_dead_indexes():
    """An index and its resident searcher refer to each other, so the many indexes
    these tests drop (pinned buffers, captured graphs) are freed only by the
    cyclic collector: run it between tests, not whenever it next happens to start."""
    yield
    gc.collect()


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native, serving
    native.lib()
    return serving


@pytest.fixture(scope="module")
def data():
    """The corpus, the queries and the whole script, drawn once and read-only."""
    rng = np.random.default_rng(2024)
    x = _dyadic(rng, N, D)
    i, j, l = PLANT
    x[j] = x[l] = x[i]
    q = _dyadic(rng, max(NQ), D)
    q[0] = x[i]
    others = np.array([p for p in range(1, N - 1) if p not in PLANT])
    first = [0, N - 1, i] + rng.choice(others, 1237 - 3, replace=False).tolist()           # 1,237 ids, first and last row
    alive = np.setdiff1d(others, first)
    known = rng.choice(alive, 300, replace=False).tolist()
    upd_ids = [_id(p) for p in known] + [_id(N + t) for t in range(20)] + [_id(known[7])]   # one known id twice
    order = rng.permutation(len(upd_ids))
    upd_ids = [upd_ids[t] for t in order]
    upd_rows = _dyadic(rng, len(upd_ids), D)
    add_ids = [_id(N + 20 + t) for t in range(100)]
    add_rows = _dyadic(rng, 100, D)
    pool = np.concatenate([np.setdiff1d(alive, known)[:200], np.array(known[:40]), np.arange(N, N + 120)])
    second = [_id(p) for p in rng.choice(pool, 50, replace=False).tolist()]
    for a in (x, q, upd_rows, add_rows):
        a.setflags(write=False)
    allowed = [_id(n) for n in range(0, N + 120, 2)] + [_id(PLANT[1]), _id(PLANT[2])]
    return {"x": x, "q": q, "first": [_id(p) for p in first], "upd": (upd_rows, upd_ids), "add": (add_rows, add_ids),
            "second": second, "allowed": allowed}


class Model:
    """What the index must equal: the surviving raw rows and ids, in order."""

    def __init__(self, x, ids):
        self.rows, self.ids = [r for r in x], list(ids)

    def remove(self, ids):
        gone = set(ids)
        keep = [t for t, i in enumerate(self.ids) if i not in gone]
        n = len(self.ids) - len(keep)
        self.rows, self.ids = [self.rows[t] for t in keep], [self.ids[t] for t in keep]
        return n

    def upsert(self, rows, ids):
        where = {i: t for t, i in enumerate(self.ids)}
        for r, i in zip(rows, ids):           # one pair after the other: the last occurrence of an id wins
            if i in where:
                self.rows[where[i]] = r
            else:
                where[i] = len(self.ids)
                self.rows.append(r)
                self.ids.append(i)

    def add(self, rows, ids):
        self.rows.extend(rows)
        self.ids.extend(ids)

    def fresh(self, S, cfg):
        index = S.HipFlatIPIndex(dict(cfg))
        index.build(np.stack(self.rows), self.ids)
        return index


def _cfg(metric, storage, online, mutable=True):
    cfg = {"dimension": D, "metric": metric, "storage_dtype": storage, "mutable": mutable}
    if online:
        cfg["online_max_batch"] = online
    return cfg


def _same_index(index, fresh, model, q, allowed, what):
    n = len(model.ids)
    # bookkeeping: size, the three id structures, the stored bits
    assert index.current_size == n == fresh.current_size == len(index._ids), what
    assert index._ids == model.ids, what
    assert index.id_map == dict(enumerate(model.ids)) == fresh.id_map, what
    assert index.reverse_id_map == {i: p for p, i in enumerate(model.ids)} == fresh.reverse_id_map, what
    assert np.array_equal(index.vectors().view(np.int32), fresh.vectors().view(np.int32)), what
    ints = torch.int32 if index.storage_dtype == torch.float32 else torch.int16
    assert torch.equal(index.index[:n].view(ints), fresh.index[:n].view(ints)), what   # the L2 column included
    # the lists: ids equal, scores equal as floats
    for nq in NQ:
        for k in KS:
            for filt in (None, allowed):
                got = index.search(q[:nq] if nq > 1 else q[0], k, filt)
                want = fresh.search(q[:nq] if nq > 1 else q[0], k, filt)
                assert got == want, (what, nq, k, filt is not None)
                assert len(got[0]) == nq and (filt is not None or len(got[0][0]) == min(k, n)), (what, nq, k)


@pytest.mark.parametrize("metric,storage,online", CONFIGS)
def test_mutated_index_equals_a_fresh_build(S, data, metric, storage, online):
    cfg = _cfg(metric, storage, online)
    ids = [_id(p) for p in range(N)]
    index = S.HipFlatIPIndex(dict(cfg))
    index.build(data["x"], ids)
    model = Model(data["x"], ids)
    q, allowed = data["q"], data["allowed"]
    what = (metric, storage, online)

    def check(step):
        _same_index(index, model.fresh(S, cfg), model, q, allowed, what + (step,))

    check("build")
    gen = index._generation
    assert index.remove(data["first"] + ["no_such_item", data["first"][5]]) == 1237 == model.remove(data["first"])
    assert index._generation == gen + 1
    check("remove")
    # the planted tie: i left, so j precedes l at equal scores
    got_ids, got_scores = index.search(q[0], 10)
    a, b = got_ids[0].index(_id(PLANT[1])), got_ids[0].index(_id(PLANT[2]))
    assert b == a + 1 and got_scores[0][a] == got_scores[0][b] and _id(PLANT[0]) not in got_ids[0], what
    assert index.remove(["no_such_item"]) == 0 and index.remove([]) == 0 and index._generation == gen + 1

    rows, uids = data["upd"]
    size = index.current_size
    index.update(rows, uids)
    model.upsert(rows, uids)
    assert index.current_size == size + 20, what                       # 300 in place (one given twice), 20 appended
    check("update")
    with pytest.raises(ValueError):
        index.update(rows[:3], uids[:2])

    index.add(*data["add"])
    model.add(*data["add"])
    check("add")

    assert index.remove(data["second"]) == 50 == model.remove(data["second"])
    check("remove 2")


def test_in_place_update_bumps_nothing_and_a_twice_stored_id_leaves_whole(S, data):
    ids = [_id(p) for p in range(200)]
    index = S.HipFlatIPIndex(_cfg("inner_product", "float32", 0))
    index.build(data["x"][:200], ids)
    index.add(data["x"][200:203], [_id(5), "no_dup", _id(5)])          # _id(5) now names three rows
    gen, ptr = index._generation, index.index.data_ptr()
    index.update(data["x"][300:302], [_id(7), _id(5)])
    assert index._generation == gen and index.index.data_ptr() == ptr and index.current_size == 203
    v = index.vectors()
    assert np.array_equal(v[7], data["x"][300]) and np.array_equal(v[202], data["x"][301])   # its last row
    assert np.array_equal(v[5], data["x"][5]) and np.array_equal(v[200], data["x"][200])
    assert index.remove([_id(5)]) == 3
    assert index._ids == ids[:5] + ids[6:] + ["no_dup"] and index._generation == gen + 1
    assert np.array_equal(index.vectors()[-1], data["x"][201])


def _searcher_lists(index, scores, pos, k):
    return [index.id_map[int(p)] for p in pos[0][:k]], [float(s) for s in scores[0][:k]]


def test_online_searcher_keeps_its_graph_over_an_update_and_drops_it_on_remove(S, data):
    cfg = _cfg("cosine", "float32", 0)
    ids = [_id(p) for p in range(N)]
    index = S.HipFlatIPIndex(dict(cfg))
    index.build(data["x"], ids)
    model = Model(data["x"], ids)
    s = index.online_searcher(8)
    q = data["q"][3]
    s.search(q, 10)
    before = _searcher_lists(index, *s.search(q, 10), 10)
    g = s._graphs[(1, 10)]
    target = _id(1234)
    assert target not in before[0]
    index.update(q * 0.5, [target])                                    # cosine: the row now scores 1 against q
    model.upsert([q * 0.5], [target])
    after = _searcher_lists(index, *s.search(q, 10), 10)
    assert s._graphs[(1, 10)] is g                                     # the same captured graph, replayed
    want = model.fresh(S, cfg).search(q, 10)
    assert after[0] == want[0][0] and after[1] == want[1][0]
    assert after[0][0] == target and after[1][0] > before[1][0]
    assert index.remove([target]) == 1 == model.remove([target])
    again = _searcher_lists(index, *s.search(q, 10), 10)
    assert s._graphs[(1, 10)] is not g                                 # dropped and captured again
    want = model.fresh(S, cfg).search(q, 10)
    assert again[0] == want[0][0] and again[1] == want[1][0] and again == before


def test_online_recommender_over_a_mutated_index(S, data):
    from rtrec_amd.models.two_tower import UserTower
    torch.manual_seed(0)
    tower = UserTower(10, embedding_dim=D, hidden_layers=[64]).cuda().eval()
    cfg = _cfg("cosine", "float32", 8)
    ids = [_id(p) for p in range(N)]
    index = S.HipFlatIPIndex(dict(cfg))
    index.build(data["x"], ids)
    model = Model(data["x"], ids)
    rec = S.OnlineRecommender(tower, index)
    x = np.random.default_rng(1).standard_normal((1, 10)).astype(np.float32)
    rec.recommend(x, k=10)
    before = rec.recommend(x, k=10)
    g = rec._graphs[(1, 10, False)]
    e = rec.embed(x).copy()
    target = _id(4321)
    assert target not in before[0][0]
    index.update(e, [target])
    model.upsert([e[0]], [target])
    after = rec.recommend(x, k=10)
    assert rec._graphs[(1, 10, False)] is g
    assert after == model.fresh(S, cfg).search(e, 10) and after[0][0][0] == target
    assert index.remove([target]) == 1 == model.remove([target])
    again = rec.recommend(x, k=10)
    assert rec._graphs[(1, 10, False)] is not g
    assert again == model.fresh(S, cfg).search(e, 10) == before


@pytest.mark.parametrize("metric,online", [("cosine", 8), ("cosine", 0), ("l2", 0)])
def test_emptied_index_answers_empty_lists_then_serves_again(S, data, metric, online):
    cfg = _cfg(metric, "float32", online)
    ids = [_id(p) for p in range(300)]
    index = S.HipFlatIPIndex(dict(cfg))
    index.build(data["x"][:300], ids)
    assert index.remove(ids) == 300 and index.current_size == 0
    assert index._ids == [] and index.id_map == {} and index.reverse_id_map == {}
    assert index.search(data["q"][:3], 10) == ([[], [], []], [[], [], []])
    assert index.search(data["q"][0], 10, filter_ids=ids) == ([[]], [[]])
    new_ids = [f"new_{t}" for t in range(40)]
    index.update(data["x"][1000:1040], new_ids)                        # unknown ids: appended
    fresh = S.HipFlatIPIndex(dict(cfg))
    fresh.build(data["x"][1000:1040], new_ids)
    assert index._ids == new_ids and index.current_size == 40
    for nq in (1, 3):
        assert index.search(data["q"][:nq], 10) == fresh.search(data["q"][:nq], 10)


@pytest.mark.parametrize("metric,storage", [("cosine", "float16"), ("l2", "float32")])
def test_save_and_load_after_mutation(S, data, tmp_path, metric, storage):
    cfg = _cfg(metric, storage, 0)
    ids = [_id(p) for p in range(1000)]
    index = S.HipFlatIPIndex(dict(cfg))
    index.build(data["x"][:1000], ids)
    index.remove(ids[::3])
    index.update(data["x"][2000:2010], ids[1:30:3])
    index.add(data["x"][3000:3005], [f"late_{t}" for t in range(5)])
    index.save(str(tmp_path / "ix"))
    loaded = S.HipFlatIPIndex({"dimension": D, "metric": metric, "storage_dtype": storage})
    loaded.load(str(tmp_path / "ix"))
    assert loaded.mutable is True                                      # it travels in the pickled config
    assert loaded.id_map == index.id_map and loaded.current_size == index.current_size
    for k in KS:
        assert loaded.search(data["q"][:8], k) == index.search(data["q"][:8], k)
    assert loaded.remove([ids[1]]) == 1


def test_non_mutable_index_still_only_warns(S, data, caplog):
    import logging
    ids = [_id(p) for p in range(500)]
    index = S.HipFlatIPIndex(_cfg("cosine", "float32", 0, mutable=False))
    index.build(data["x"][:500], ids)
    v, gen = index.vectors(), index._generation
    with caplog.at_level(logging.WARNING, logger="rtrec_amd.retrieval"):
        assert index.update(data["x"][600:602], ids[:2]) is None
        assert index.remove(ids[:100]) is None
    assert "Flat index doesn't support direct updates. Consider periodic rebuilds." in caplog.text
    assert "Flat index doesn't support removal. Consider periodic rebuilds." in caplog.text
    assert np.array_equal(index.vectors(), v) and index.current_size == 500 and index._generation == gen
    assert index._ids == ids


def test_engine_clears_its_cache_on_upsert_and_remove(S, data):
    engine = S.RetrievalEngine({"index_type": "hip_flat", "embedding_dim": D, "top_k": 10,
                                "hip_flat": {"metric": "cosine", "mutable": True}})
    ids = [_id(p) for p in range(1000)]
    engine.build_index(data["x"][:1000], ids)
    q = data["q"][5]
    first = engine.retrieve(q)
    assert engine.retrieve(q)[2]["cache_hit"] is True
    target = _id(777)
    assert target not in first[0][0]
    engine.update_index(q[None, :] * 2.0, [target], upsert=True)
    got = engine.retrieve(q)
    assert got[2]["cache_hit"] is False and got[0][0][0] == target and engine.index.current_size == 1000
    assert engine.retrieve(q)[2]["cache_hit"] is True
    assert engine.remove_items([target]) == 1
    got = engine.retrieve(q)
    assert got[2]["cache_hit"] is False and got[0] == first[0] and engine.index.current_size == 999
    engine.update_index(q[None, :], ["appended"])                     # the default still appends
    assert engine.index.current_size == 1000 and engine.retrieve(q)[0][0][0] == "appended"
