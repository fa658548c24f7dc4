"""Seen-item exclusion on the online search path: rt_flatip_topk_online_lists
(the scan of csrc/topk_online.hip reading CSR exclusion lists itself), and what
is built on it — ``OnlineSearcher.search(exclude=)``, ``HipFlatIPIndex.search``
/ ``RetrievalEngine.retrieve(exclude_ids=)``, ``OnlineRecommender.recommend(
exclude_items=, exclude_seen=)``.

The yardstick is the C oracle: ``flat_ip_search(..., exclude_bits=
exclusion_bitmap(...))``. Scores bit-equal, ids equal, pads (-FLT_MAX, -1) —
np.array_equal throughout, as tests/test_gpu_topk_online.py compares.

Shapes are the smallest at which each path runs: 4,097 rows (17 blocks of one
256-row tile, the last ragged), 1,000 rows (few or none left), and 600,013 rows
at d = 8, where rows_per_block is 1,172 — five tiles per block, the last
ragged — so a block's cursors cross tile boundaries, a whole tile and a whole
block can be excluded, and a 100,000-entry list puts about 195 entries into
every block (rounds of more than 64 entries per tile included)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NEG = -np.finfo(np.float32).max
BIG_NX, BIG_D = 600_013, 8


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


@pytest.fixture(scope="module")
def S(K):
    from rtrec_amd import serving
    return serving


def _bits(t):
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


def _oracle(q_t, x_t, k, excluded=None, id_offset=0):
    """q_t, x_t: CPU tensors in the storage dtype; excluded: per query, positions."""
    qa, code = _bits(q_t)
    xa, _ = _bits(x_t)
    bm = None if excluded is None else orc.exclusion_bitmap(q_t.shape[0], x_t.shape[0],
                                                            [np.asarray(e, np.int64).tolist() for e in excluded])
    return orc.flat_ip_search(qa, xa, k, exclude_bits=bm, id_offset=id_offset, dtype_code=code, nthreads=16)


def _csr(lists, rows=None):
    """Per-row position lists -> a source (offsets, items[, rows]) on the device."""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(e) for e in lists], out=off[1:])
    items = np.concatenate([np.asarray(e, np.int32) for e in lists]) if off[-1] else np.zeros(0, np.int32)
    src = (torch.from_numpy(off).cuda(), torch.from_numpy(items.astype(np.int32)).cuda())
    if rows is not None:
        src += (torch.tensor(rows, dtype=torch.int64, device="cuda"),)
    return src


def _assert_equal(got, rs, ri, what=""):
    torch.cuda.synchronize()
    gs = got[0].cpu().numpy() if isinstance(got[0], torch.Tensor) else np.asarray(got[0])
    gi = got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else np.asarray(got[1])
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs, rs), what


def _none_excluded(gi, excluded, id_offset=0):
    for q, e in enumerate(excluded):
        assert not (set((gi[q][gi[q] >= 0] - id_offset).tolist()) & set(int(i) for i in e)), q


# ---- 1. the current top-k excluded ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_case():
    rng = np.random.default_rng(7)
    q = rng.standard_normal((8, 64)).astype(np.float32)
    x = rng.standard_normal((4097, 64)).astype(np.float32)
    return torch.from_numpy(q), torch.from_numpy(x)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_current_topk_excluded(K, dtype):
    """Each query's list is its own current top-k, then its neighbour's: the
    result is the next k, with ids offset by id_offset and lists in positions."""
    q32, x32 = _small_case()
    qt, xt = q32.to(dtype), x32.to(dtype)
    k, off = 50, 5_000_000
    _, top = _oracle(qt, xt, k)
    qd, xd = qt.cuda(), xt.cuda()
    for shift in (0, 1):
        excluded = [np.sort(top[(qi + shift) % 8]) for qi in range(8)]
        rs, ri = _oracle(qt, xt, k, excluded, id_offset=off)
        got = K.flatip_topk_online(qd, xd, k, id_offset=off, exclude_lists=_csr(excluded))
        _assert_equal(got, rs, ri, f"{dtype} shift={shift}")
        _none_excluded(ri, excluded, off)
        assert (ri >= off).all()


# ---- 2./3. block and tile edges, a long list: 600,013 rows at d = 8 --------------
@functools.lru_cache(maxsize=None)
def _big_case():
    """Small-integer rows (exact scores, many ties) with PLANTED rows that beat
    every other row for every query (all-positive queries, planted rows all 7)."""
    from rtrec_amd import kernels
    rng = np.random.default_rng(11)
    x = rng.integers(-3, 4, size=(BIG_NX, BIG_D)).astype(np.float32)
    q = rng.integers(1, 4, size=(8, BIG_D)).astype(np.float32)
    blocks, rpb = kernels.flatip_topk_online_plan(8, BIG_NX, BIG_D, F32, 128)
    assert rpb == 1172 and blocks == 512 and (BIG_NX - 511 * rpb) % 256 != 0
    planted = [0, BIG_NX - 1, 7 * rpb, 8 * rpb - 1, 3 * rpb + 255, 3 * rpb + 256]
    planted += list(range(100 * rpb + 512, 100 * rpb + 768))      # every row of one tile
    planted += list(range(200 * rpb, 201 * rpb))                  # every row of one block
    planted = np.unique(np.asarray(planted, np.int64))
    x[planted] = 7.0
    return torch.from_numpy(q), torch.from_numpy(x), planted, rng.integers(0, BIG_NX, size=(8, 10))


@functools.lru_cache(maxsize=None)
def _big_device():
    q, x, _, _ = _big_case()
    return q.cuda(), x.cuda()


def test_block_and_tile_edges(K):
    q, x, planted, extra = _big_case()
    qd, xd = _big_device()
    # without exclusion the planted rows fill every top-128 (the lower positions win the ties)
    _, plain = _oracle(q[:1], x, 128)
    assert set(plain[0].tolist()) <= set(planted.tolist())
    excluded = [np.unique(np.concatenate([planted, extra[qi]])) for qi in range(8)]
    rs, ri = _oracle(q, x, 128, excluded)
    _none_excluded(ri, excluded)
    src = _csr(excluded)
    for nq in (1, 8):
        for k in (128, 1):
            got = K.flatip_topk_online(qd[:nq], xd, k, exclude_lists=(src[0][:nq + 1], src[1]))
            _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nq={nq} k={k}")


def test_long_lists(K):
    """100,000 random positions per query, different per query: about 195 per
    block, tiles with several entries, every block's cursor crossing all its tiles."""
    q, x, _, _ = _big_case()
    qd, xd = _big_device()
    rng = np.random.default_rng(13)
    excluded = [np.unique(rng.integers(0, BIG_NX, size=100_000)) for _ in range(8)]
    rs, ri = _oracle(q, x, 100, excluded)
    got = K.flatip_topk_online(qd, xd, 100, exclude_lists=_csr(excluded))
    _assert_equal(got, rs, ri, "long lists")
    _none_excluded(ri, excluded)


# ---- 4. few or none left ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _thousand():
    rng = np.random.default_rng(17)
    return (torch.from_numpy(rng.standard_normal((8, 32)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((1000, 32)).astype(np.float32)))


def test_few_or_none_left(K):
    q, x = _thousand()
    qd, xd = q.cuda(), x.cuda()
    everything = np.arange(1000)
    all_but_3 = np.delete(everything, [0, 511, 999])
    cases = {
        "all but 3": [all_but_3] * 8,
        "every row": [everything] * 8,
        "empty next to full": [everything if qi % 2 else np.zeros(0, np.int64) for qi in range(8)],
    }
    for name, excluded in cases.items():
        rs, ri = _oracle(q, x, 10, excluded)
        got = K.flatip_topk_online(qd, xd, 10, exclude_lists=_csr(excluded))
        _assert_equal(got, rs, ri, name)
    rs, ri = _oracle(q, x, 10, cases["all but 3"])
    assert (ri[:, 3:] == -1).all() and (rs[:, 3:] == NEG).all() and (ri[:, :3] >= 0).all()
    rs, ri = _oracle(q, x, 10, cases["every row"])
    assert (ri == -1).all() and (rs == NEG).all()


# ---- 5. the row convention -------------------------------------------------------------
def test_row_convention(K):
    """rows[q] picks the CSR row; -1 and n_rows mean no exclusions; entries at and
    past nx are ignored; duplicated entries are harmless."""
    q32, x32 = _small_case()
    nx, k = x32.shape[0], 50
    _, top = _oracle(q32, x32, k)
    csr_rows = [
        np.sort(np.concatenate([top[0], top[0][:7]])),                    # duplicates
        np.concatenate([np.sort(top[1]), [nx, nx + 5]]),                  # trailing entries outside the corpus
        np.sort(top[5][:9]),
    ]
    rows = [1, 1, -1, 3, 0, 2, 0, 2]                                      # n_rows = 3
    excluded = [np.zeros(0, np.int64) if not 0 <= r < 3 else csr_rows[r][csr_rows[r] < nx] for r in rows]
    rs, ri = _oracle(q32, x32, k, excluded)
    got = K.flatip_topk_online(q32.cuda(), x32.cuda(), k, exclude_lists=_csr(csr_rows, rows))
    _assert_equal(got, rs, ri, "rows")
    assert np.array_equal(ri[2], top[2]) and np.array_equal(ri[3], top[3])  # no exclusions for -1 and n_rows
    _none_excluded(ri, excluded)


# ---- 6. two sources ----------------------------------------------------------------------
@pytest.mark.parametrize("how", ["disjoint", "overlapping", "identical"])
def test_two_sources(K, how):
    q32, x32 = _small_case()
    k = 50
    _, top = _oracle(q32, x32, 100)
    if how == "disjoint":
        a, b = [np.sort(t[:30]) for t in top], [np.sort(t[30:70]) for t in top]
    elif how == "overlapping":
        a, b = [np.sort(t[:40]) for t in top], [np.sort(t[20:60]) for t in top]
    else:
        a = b = [np.sort(t[:50]) for t in top]
    union = [np.union1d(x, y) for x, y in zip(a, b)]
    rs, ri = _oracle(q32, x32, k, union)
    # the second source is one shared CSR looked up through rows, as a resident seen-items CSR is
    order = [3, 0, 7, 1, 6, 2, 5, 4]
    b_csr = [b[order.index(r)] for r in range(8)]
    got = K.flatip_topk_online(q32.cuda(), x32.cuda(), k, exclude_lists=[_csr(a), _csr(b_csr, order)])
    _assert_equal(got, rs, ri, how)
    _none_excluded(ri, union)


# ---- 7. no lists ----------------------------------------------------------------------------
def test_no_lists_is_the_old_entry_bit_for_bit(K):
    from rtrec_amd import native
    q32, x32 = _small_case()
    for dtype in (F32, F16):
        qd, xd = q32.to(dtype).cuda(), x32.to(dtype).cuda()
        want = K.flatip_topk_online(qd, xd, 50, id_offset=9)
        s = torch.empty((8, 50), dtype=torch.float32, device="cuda")
        i = torch.empty((8, 50), dtype=torch.int64, device="cuda")
        ws = torch.empty(native.lib().rt_flatip_topk_online_workspace_bytes(8, 4097, 64, native.dtype_code(dtype), 50),
                         dtype=torch.uint8, device="cuda")
        native.call("rt_flatip_topk_online_lists", native.ptr(qd), 8, native.ptr(xd), 4097, 64,
                    native.dtype_code(dtype), 50, None, 0, 9, native.ptr(s), native.ptr(i), native.ptr(ws),
                    ws.numel(), native.stream_of(qd))
        torch.cuda.synchronize()
        assert torch.equal(s, want[0]) and torch.equal(i, want[1])
        # a source without items is no source
        got = K.flatip_topk_online(qd, xd, 50, id_offset=9, exclude_lists=_csr([[]] * 8))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 8. the searcher ---------------------------------------------------------------------------
def _index(S, x, **cfg):
    index = S.HipFlatIPIndex({"dimension": x.shape[1], "metric": "inner_product", **cfg})
    index.build(x, [f"item_{i}" for i in range(x.shape[0])])
    return index


@pytest.mark.parametrize("graph", ["1", "0"])
def test_searcher_replays_one_graph_for_every_list_length(S, monkeypatch, graph):
    monkeypatch.setenv("RTREC_ONLINE_GRAPH", graph)
    q32, x32 = _small_case()
    nx, nq, k, cap = x32.shape[0], 3, 50, 512
    index = _index(S, x32.numpy())
    searcher = index.online_searcher(8, max_exclude=cap)
    rng = np.random.default_rng(19)
    q = q32[:nq]
    rs, ri = _oracle(q, x32, k)
    _assert_equal(searcher.search(q.numpy(), k), rs, ri, "no lists")
    n_plain = len(searcher._graphs)
    n_with = None
    for total in (0, 1, 166, cap, cap + 1):
        sizes = [total // nq + (1 if r < total % nq else 0) for r in range(nq)]
        excluded = [rng.choice(nx, size=n, replace=False) for n in sizes]
        # unsorted and duplicated on the way in: the searcher sorts and de-duplicates
        given = [np.concatenate([e, e[:2]]) for e in excluded]
        rs, ri = _oracle(q, x32, k, excluded)
        got = searcher.search(q.numpy(), k, exclude=given)
        _assert_equal(got, rs, ri, f"graph={graph} total={total}")
        if n_with is None:
            n_with = len(searcher._graphs)
        assert len(searcher._graphs) == n_with, total   # cap + 1: the fallback captures nothing either
    assert n_with == (n_plain + 1 if graph == "1" else 0)
    # without lists: the graph from before the lists, and its result
    rs, ri = _oracle(q, x32, k)
    _assert_equal(searcher.search(q.numpy(), k), rs, ri, "no lists again")
    assert len(searcher._graphs) == n_with
    with pytest.raises(ValueError):
        searcher.search(q.numpy(), k, exclude=[[1]])         # one list for three queries


# ---- 9. index and engine ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["online", "default", "l2"])
def test_index_search_exclude_ids(S, mode):
    q32, x32 = _small_case()
    x, q, nx, k = x32.numpy(), q32.numpy()[:4], x32.shape[0], 20
    cfg = {"online": {"online_max_batch": 8}, "default": {}, "l2": {"metric": "l2"}}[mode]
    index = _index(S, x, **cfg)
    rng = np.random.default_rng(23)
    if mode == "l2":
        _, top = orc.flat_l2_search(q, x, k, nthreads=16)
    else:
        _, top = _oracle(q32[:4], x32, k)
    excluded = [np.union1d(top[qi][::2], rng.choice(nx, size=30, replace=False)) for qi in range(4)]
    ex_ids = [[f"item_{p}" for p in e] + ["no_such_item"] for e in excluded]
    if mode == "l2":   # the oracle has no masked L2 search: the surviving rows, positions mapped back
        want = []
        for qi in range(4):
            keep = np.setdiff1d(np.arange(nx), excluded[qi])
            _, ri = orc.flat_l2_search(q[qi:qi + 1], x[keep], k, nthreads=16)
            want.append(keep[ri[0]])
    else:
        want = _oracle(q32[:4], x32, k, excluded)[1]
    ids, scores = index.search(q, k, exclude_ids=ex_ids)
    for qi in range(4):
        assert len(ids[qi]) == k == len(scores[qi])
        assert ids[qi] == [f"item_{p}" for p in want[qi]], (mode, qi)
        assert not set(ids[qi]) & set(ex_ids[qi])
    # one flat list serves every query
    flat = ex_ids[0]
    ids1, _ = index.search(q, k, exclude_ids=flat)
    assert ids1[0] == ids[0] and all(not set(r) & set(flat) for r in ids1) and all(len(r) == k for r in ids1)
    # with an allow-list as well: a subset of it, nothing excluded
    allowed = [f"item_{p}" for p in range(0, nx, 2)]
    ids2, _ = index.search(q, k, filter_ids=allowed, exclude_ids=ex_ids)
    for qi in range(4):
        assert set(ids2[qi]) <= set(allowed) and not set(ids2[qi]) & set(ex_ids[qi])
    if mode == "online":
        assert index._online is not None and (4, k, True) in index._online._graphs


def test_engine_retrieve_skips_the_cache(S):
    q32, x32 = _small_case()
    eng = S.RetrievalEngine({"index_type": "hip_flat", "embedding_dim": 64, "top_k": 10,
                             "hip_flat": {"metric": "inner_product", "online_max_batch": 8}})
    eng.build_index(x32.numpy(), [f"item_{i}" for i in range(x32.shape[0])])
    q = q32.numpy()[:1]
    ids, _, m = eng.retrieve(q, k=10)
    assert not m["cache_hit"] and len(eng.cache) == 1
    ex = ids[0][:5]
    ids2, _, m2 = eng.retrieve(q, k=10, exclude_ids=ex)
    assert not m2["cache_hit"] and len(eng.cache) == 1 and eng.cache_hits == 0   # neither read nor filled
    assert len(ids2[0]) == 10 and not set(ids2[0]) & set(ex) and ids2[0][:5] == ids[0][5:]
    want = _oracle(q32[:1], x32, 10, [[int(i.split("_")[1]) for i in ex]])[1]
    assert ids2[0] == [f"item_{p}" for p in want[0]]
    ids3, _, m3 = eng.retrieve(q, k=10)
    assert m3["cache_hit"] and ids3 == ids


# ---- 10. the recommender ---------------------------------------------------------------------------
def test_recommender_exclude_seen_and_items(S):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    n, d, users, k = 1000, 128, 64, 20
    rng = np.random.default_rng(29)
    x = rng.standard_normal((n, d)).astype(np.float32)
    item_ids = [f"item_{i}" for i in range(n)]
    torch.manual_seed(0)
    # the C2 user tower (3 features, hidden [256, 128]), served by id from a resident table
    model = TwoTowerModel(UserTower(3, d, [256, 128]), ItemTower(20, d, [64], use_content_embedding=False)).cuda()
    table = torch.from_numpy(rng.standard_normal((users, 3)).astype(np.float32)).cuda()
    index = S.HipFlatIPIndex({"dimension": d, "metric": "inner_product", "mutable": True})
    index.build(x, item_ids)
    rec = S.OnlineRecommender(model, index, user_table=table)
    uids = np.asarray([5, 17, 5, 63, 0])
    with pytest.raises(ValueError, match="set_seen"):
        rec.recommend(user_ids=uids, k=k, exclude_seen=True)
    histories = [[f"item_{p}" for p in rng.choice(n, size=int(rng.integers(0, 200)), replace=False)] + ["gone"]
                 for _ in range(users)]
    rec.set_seen(histories)
    with pytest.raises(ValueError, match="user_ids"):
        rec.recommend(table[:2].cpu().numpy(), k=k, exclude_seen=True)
    e = torch.from_numpy(rec.embed(user_ids=uids).copy())
    xt = torch.from_numpy(x)

    def positions(ids, alive):
        pos = {i: p for p, i in enumerate(alive)}
        return [pos[i] for i in ids if i in pos]

    def check(alive, xs, exclude_items, what):
        seen = [positions(histories[u], alive) for u in uids]
        extra = [positions(exclude_items, alive)] * len(uids) if exclude_items else [[]] * len(uids)
        excluded = [np.union1d(a, b).astype(np.int64) for a, b in zip(seen, extra)]
        rs, ri = _oracle(e, xs, k, excluded)
        ids, scores = rec.recommend(user_ids=uids, k=k, exclude_seen=True, exclude_items=exclude_items)
        for qi, u in enumerate(uids):
            assert ids[qi] == [alive[p] for p in ri[qi]], (what, qi)
            assert np.array_equal(np.asarray(scores[qi], np.float32), rs[qi]), (what, qi)
            assert not set(ids[qi]) & set(histories[u]) and not set(ids[qi]) & set(exclude_items or ())
        return ids

    first = check(item_ids, xt, None, "seen")
    assert (len(uids), k, True, False, True) in rec._graphs
    check(item_ids, xt, None, "seen, replayed")
    check(item_ids, xt, [i for row in first for i in row[:3]], "seen and items")
    assert (len(uids), k, True, True, True) in rec._graphs
    # a call outside the resident range honours both kinds
    ids, _ = rec.recommend(user_ids=uids, k=200, exclude_seen=True, exclude_items=first[0][:3])
    for qi, u in enumerate(uids):
        assert len(ids[qi]) == 200 and not set(ids[qi]) & (set(histories[u]) | set(first[0][:3]))
    # remove: positions move, the CSR is mapped again from the kept ids
    gone = set(item_ids[10:400:7]) | set(first[0][:2])
    index.remove(list(gone))
    alive = [i for i in item_ids if i not in gone]
    keep = np.asarray([p for p, i in enumerate(item_ids) if i not in gone])
    check(alive, torch.from_numpy(x[keep]), None, "after remove")
    check(alive, torch.from_numpy(x[keep]), alive[:4], "after remove, with items")
