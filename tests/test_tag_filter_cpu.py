"""Host side of the category filter (rt_flatip_topk_online_tags,
rt_ivf_topk_tags, rt_tag_filter_bitmap): the symbols and the struct, every
status code returned before any device work (the pointers below are fakes,
never dereferenced), the eligibility rule of the tests' own reference on
hand-written cases, the counts the shared fixture was chosen for, and the
ValueErrors of the Python wrappers. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _tag_filter_ref as tref

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_WORKSPACE = 0, -1, -2, -3
BIG = 1 << 40


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    nat.lib()
    return nat


def _filter(nat, item_tags=8, any_of=8, none_of=8):
    f = nat.TagFilter()
    f.item_tags, f.any_of, f.none_of = item_tags, any_of, none_of
    return ctypes.byref(f)


def _lists(nat, n):
    arr = (nat.ExclusionLists * max(n, 1))()
    for a in arr:
        a.offsets, a.items, a.n_rows, a.rows = 16, 16, 4, None
    return arr


def _flat(nat, flt, n_lists=0, nq=1, nx=1000, d=128, code=0, k=10, ws=256, ws_bytes=BIG, q=16, x=16, id_offset=0):
    return nat.lib().rt_flatip_topk_online_tags(q, nq, x, nx, d, code, k, _lists(nat, n_lists), n_lists, flt,
                                                id_offset, 16, 16, ws, ws_bytes, None)


def _flat_lists(nat, n_lists=0, nq=1, nx=1000, d=128, code=0, k=10, ws=256, ws_bytes=BIG, q=16, x=16, id_offset=0):
    return nat.lib().rt_flatip_topk_online_lists(q, nq, x, nx, d, code, k, _lists(nat, n_lists), n_lists, id_offset,
                                                 16, 16, ws, ws_bytes, None)


def _ivf(nat, flt, list_len=16, n_pos=1000, n_lists=0, nq=1, nx=1000, d=128, code=0, k=10, nprobe=4, ws=256,
         ws_bytes=BIG, mlr=300):
    return nat.lib().rt_ivf_topk_tags(16, nq, 16, nx, d, code, 16, 8, list_len, n_pos, 16, 16, nprobe, mlr, k,
                                      _lists(nat, n_lists), n_lists, flt, 16, 16, ws, ws_bytes, None)


def _ivf_lists(nat, list_len=16, n_pos=1000, n_lists=0, nq=1, nx=1000, d=128, code=0, k=10, nprobe=4, ws=256,
               ws_bytes=BIG, mlr=300):
    lib = nat.lib()
    if list_len is None:
        return lib.rt_ivf_topk_lists(16, nq, 16, nx, d, code, 16, 8, 16, 16, nprobe, mlr, k, _lists(nat, n_lists),
                                     n_lists, 16, 16, ws, ws_bytes, None)
    return lib.rt_ivf_topk_lists_lens(16, nq, 16, nx, d, code, 16, 8, list_len, n_pos, 16, 16, nprobe, mlr, k,
                                      _lists(nat, n_lists), n_lists, 16, 16, ws, ws_bytes, None)


def test_symbols_and_struct(native):
    for name in ("rt_flatip_topk_online_tags", "rt_ivf_topk_tags", "rt_tag_filter_bitmap"):
        assert hasattr(native.lib(), name), name
        assert name in native.SIGNATURES
    assert [f for f, _ in native.TagFilter._fields_] == ["item_tags", "any_of", "none_of"]
    assert ctypes.sizeof(native.TagFilter) == 24
    assert [getattr(native.TagFilter, f).offset for f, _ in native.TagFilter._fields_] == [0, 8, 16]


def test_flat_filter_refusals(native):
    assert _flat(native, _filter(native, item_tags=None)) == RT_ERR_INVALID           # rows exist, no tags
    for bad in ({"item_tags": 20}, {"any_of": 20}, {"none_of": 20}, {"item_tags": 4}):
        assert _flat(native, _filter(native, **bad)) == RT_ERR_INVALID, bad           # 8-byte alignment
    # the filter's refusals come first: a call that is invalid both ways reports the filter
    assert _flat(native, _filter(native, item_tags=None), nq=9) == RT_ERR_INVALID
    # NULL masks are all 0, and an empty corpus needs no tags
    assert _flat(native, _filter(native, any_of=None, none_of=None), ws=None) == RT_ERR_WORKSPACE
    assert _flat(native, _filter(native, item_tags=None), nx=0, x=None, ws=None) == RT_ERR_WORKSPACE


@pytest.mark.parametrize("with_filter", [True, False])
def test_flat_every_other_refusal_is_the_lists_entrys(native, with_filter):
    """With a well-formed filter, or filter == NULL (which forwards), the status
    is rt_flatip_topk_online_lists'."""
    flt = _filter(native) if with_filter else None

    def both(**kw):
        new, old = _flat(native, flt, **kw), _flat_lists(native, **kw)
        assert new == old, kw
        return new

    assert both(n_lists=-1) == RT_ERR_INVALID
    assert both(n_lists=3) == RT_ERR_UNSUPPORTED
    assert both(nq=9) == RT_ERR_UNSUPPORTED
    assert both(k=129) == RT_ERR_UNSUPPORTED
    assert both(d=130) == RT_ERR_UNSUPPORTED
    assert both(nx=1 << 32) == RT_ERR_UNSUPPORTED
    assert both(id_offset=-1) == RT_ERR_UNSUPPORTED
    assert both(nq=-1) == RT_ERR_INVALID
    assert both(k=0) == RT_ERR_INVALID
    assert both(code=5) == RT_ERR_INVALID
    assert both(q=None) == RT_ERR_INVALID
    assert both(x=None) == RT_ERR_INVALID
    assert both(q=24) == RT_ERR_INVALID
    assert both(ws=None) == RT_ERR_WORKSPACE
    assert both(n_lists=2, ws=None) == RT_ERR_WORKSPACE
    assert both(nq=0, ws=None, ws_bytes=0) == RT_OK
    for nq, nx, k in ((1, 1000, 50), (8, 10**6, 128)):
        need = native.lib().rt_flatip_topk_online_workspace_bytes(nq, nx, 128, 0, k)
        assert both(nq=nq, nx=nx, k=k, ws_bytes=need - 1) == RT_ERR_WORKSPACE


def test_ivf_filter_refusals(native):
    assert _ivf(native, _filter(native, item_tags=None)) == RT_ERR_INVALID
    assert _ivf(native, _filter(native, item_tags=None), list_len=None, n_pos=0) == RT_ERR_INVALID   # nx positions
    for bad in ({"item_tags": 20}, {"any_of": 20}, {"none_of": 20}):
        assert _ivf(native, _filter(native, **bad)) == RT_ERR_INVALID, bad
    assert _ivf(native, _filter(native, item_tags=None), nprobe=129) == RT_ERR_INVALID   # the filter first
    # lists with slack and no valid position: no tags needed
    assert _ivf(native, _filter(native, item_tags=None), n_pos=0, ws=None) == RT_ERR_WORKSPACE
    assert _ivf(native, _filter(native, any_of=None, none_of=None), ws=None) == RT_ERR_WORKSPACE


@pytest.mark.parametrize("with_filter", [True, False])
@pytest.mark.parametrize("slack", [True, False])
def test_ivf_every_other_refusal_is_the_lists_entrys(native, with_filter, slack):
    """list_len == NULL: rt_ivf_topk_lists (n_pos ignored); else rt_ivf_topk_lists_lens."""
    flt = _filter(native) if with_filter else None
    base = {} if slack else {"list_len": None, "n_pos": -5}

    def both(**kw):
        a = dict(base, **kw)
        new, old = _ivf(native, flt, **a), _ivf_lists(native, **a)
        assert new == old, a
        return new

    assert both(n_lists=-1) == RT_ERR_INVALID
    assert both(n_lists=3) == RT_ERR_UNSUPPORTED
    assert both(k=129) == RT_ERR_UNSUPPORTED
    assert both(nprobe=129) == RT_ERR_UNSUPPORTED
    assert both(nq=65536) == RT_ERR_UNSUPPORTED
    assert both(d=130) == RT_ERR_UNSUPPORTED
    assert both(nx=(1 << 31) - 1) == RT_ERR_UNSUPPORTED
    assert both(nq=-1) == RT_ERR_INVALID
    assert both(k=0) == RT_ERR_INVALID
    assert both(nprobe=0) == RT_ERR_INVALID
    assert both(code=7) == RT_ERR_INVALID
    assert both(ws=None) == RT_ERR_WORKSPACE
    assert both(ws_bytes=255) == RT_ERR_WORKSPACE
    assert both(nq=0, ws=None, ws_bytes=0) == RT_OK
    if slack:
        assert both(n_pos=-1) == RT_ERR_INVALID
        assert both(n_pos=(1 << 31) - 1) == RT_ERR_UNSUPPORTED


def test_bitmap_status_codes(native):
    f = native.lib().rt_tag_filter_bitmap
    assert f(None, 100, 8, 8, 2, 64, 4, 0, None) == RT_ERR_INVALID      # items, no tags
    assert f(20, 100, 8, 8, 2, 64, 4, 0, None) == RT_ERR_INVALID        # alignment
    assert f(8, 100, 20, 8, 2, 64, 4, 0, None) == RT_ERR_INVALID
    assert f(8, 100, 8, 20, 2, 64, 4, 0, None) == RT_ERR_INVALID
    assert f(8, 100, 8, 8, 2, 66, 4, 0, None) == RT_ERR_INVALID
    assert f(8, 100, 8, 8, 2, 64, 3, 0, None) == RT_ERR_INVALID         # words < ceil(100 / 32)
    assert f(8, 100, 8, 8, 2, None, 4, 1, None) == RT_ERR_INVALID
    assert f(8, -1, 8, 8, 2, 64, 4, 0, None) == RT_ERR_INVALID
    assert f(8, 100, 8, 8, -1, 64, 4, 0, None) == RT_ERR_INVALID
    assert f(8, 100, 8, 8, 0, None, 4, 0, None) == RT_OK                # no queries
    assert f(None, 0, None, None, 3, None, 0, 0, None) == RT_OK         # no words


# ---- the reference's eligibility rule, hand-written ----
def test_reference_eligibility_rule():
    B = lambda *bits: sum(1 << b for b in bits)   # noqa: E731
    tags = np.array([0, B(0), B(1), B(0, 1), B(63), B(2, 63)], dtype=np.uint64)
    any_of = np.array([0, B(0), B(0), B(0, 1), B(63), 0, B(1), B(5)], dtype=np.uint64)
    none_of = np.array([0, 0, B(1), B(1), 0, B(63), B(1), 0], dtype=np.uint64)
    want = np.array([
        [1, 1, 1, 1, 1, 1],   # no masks: nothing filtered, the untagged item included
        [0, 1, 0, 1, 0, 0],   # any_of bit 0: an untagged item passes no non-zero any_of
        [0, 1, 0, 0, 0, 0],   # ... and none_of bit 1 drops the item that has both
        [0, 1, 0, 0, 0, 0],   # any_of {0, 1} with none_of {1}: the overlap excludes
        [0, 0, 0, 0, 1, 1],   # bit 63
        [1, 1, 1, 1, 0, 0],   # any_of == 0 with none_of bit 63: the untagged item fails no none_of
        [0, 0, 0, 0, 0, 0],   # any_of == none_of: nothing can pass
        [0, 0, 0, 0, 0, 0],   # a category no item has
    ], dtype=bool)
    got = tref.eligible(tags, any_of, none_of)
    assert got.dtype == bool and np.array_equal(got, want)
    bits = tref.filter_bits(tags, any_of, none_of)
    assert bits.shape == (8, 1) and bits.dtype == np.uint32
    assert [int(b) for b in bits[:, 0]] == [int(sum((not e) << p for p, e in enumerate(row))) for row in want]
    other = np.full((8, 1), 1 << 1, dtype=np.uint32)
    assert np.array_equal(tref.filter_bits(tags, any_of, none_of, other=other), bits | np.uint32(2))


def test_fixture_tags_and_masks():
    t = tref.fixture_tags(8192)
    assert t.dtype == np.uint64 and t[0] == 0 and t[11] == 0 and t[1] == (1 << 1) | (1 << 8)
    assert t[3] == (1 << 3) | (1 << 10) | (1 << 63)
    assert int((t >> np.uint64(63)).sum()) == 6
    a, n = tref.fixture_masks(256)
    assert a[8] == 1 << 1 and n[8] == 1 << 10 and len(set(zip(a.tolist(), n.tolist()))) == 35


def test_fixture_counts():
    """What the k cases of the GPU tests rest on: at (nprobe 4, k 20) 255 queries
    fill k and one pads; at (4, 100) every query pads; at (64, 100) none does."""
    c4, c64 = tref.eligible_in_probed(4), tref.eligible_in_probed(64)
    assert (int(c4.min()), int(c4.max()), int(np.median(c4))) == (17, 97, 53)
    assert int((c4 >= 20).sum()) == 255 and int((c4 < 100).sum()) == 256
    assert 850 <= int(c64.min()) and int(c64.max()) <= 852
    f = tref.ivf_fixture()
    ok = tref.eligible(f["tags"], f["any_of"], f["none_of"])
    assert np.array_equal(c64, ok.sum(axis=1))   # nprobe = nlist: the whole corpus


def test_wrapper_value_errors(native):
    from rtrec_amd import kernels
    q, x = torch.zeros(2, 128), torch.zeros(100, 128)
    tags = torch.zeros(100, dtype=torch.int64)
    m = torch.zeros(2, dtype=torch.int64)
    bits = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        kernels.flatip_topk_online(q, x, 10, exclude_bits=bits, tag_filter=(tags, m, m))
    with pytest.raises(ValueError, match="item_tags, any_of, none_of"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags, m))
    with pytest.raises(ValueError, match="item_tags"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(None, m, m))
    with pytest.raises(TypeError, match="64-bit"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags.to(torch.int32), m, m))
    with pytest.raises(TypeError, match="64-bit"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags, m.to(torch.int32), m))
    with pytest.raises(ValueError, match="item_tags"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags[:99], m, m))
    with pytest.raises(ValueError, match="none_of"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags, m, m[:1]))
    # a well-formed filter of CPU tensors: refused like every CPU tensor, no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.flatip_topk_online(q, x, 10, tag_filter=(tags, m, None))
    off = torch.zeros(5, dtype=torch.int64)
    rp = torch.zeros(100, dtype=torch.int32)
    pr = torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="mutually exclusive"):
        kernels.ivf_topk(q, x, off, rp, pr, 100, 10, exclude_bits=bits, tag_filter=(tags, m, m))
    with pytest.raises(ValueError, match="item_tags"):
        kernels.ivf_topk(q, x, off, rp, pr, 100, 10, tag_filter=(tags[:50], m, m))
    with pytest.raises(TypeError, match="64-bit"):
        kernels.tag_filter_bitmap(tags.to(torch.int32), m, m, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.tag_filter_bitmap(tags, m, m, 2)


def test_index_refusals_at_construction():
    """The sharded index and the L2 mode do not serve category filters; the
    vocabulary holds at most 64 distinct names."""
    from rtrec_amd.serving import retrieval as R
    with pytest.raises(ValueError, match="HipFlatIPIndex, HipIVFFlatIndex, HipMutableIVFFlatIndex"):
        R.HipShardedFlatIPIndex({"dimension": 32, "categories": ["a", "b"]})
    sharded = R.HipShardedFlatIPIndex({"dimension": 32})
    with pytest.raises(ValueError, match="single-GPU"):
        sharded.search(np.zeros((1, 32), np.float32), 5, filter_categories=["a"])
    with pytest.raises(ValueError, match="single-GPU"):
        sharded.search(np.zeros((1, 32), np.float32), 5, exclude_categories=["a"])
    with pytest.raises(ValueError, match="L2"):
        R.HipFlatIPIndex({"dimension": 32, "metric": "l2", "categories": ["a"]})
    with pytest.raises(ValueError, match="at most 64"):
        R.HipFlatIPIndex({"dimension": 32, "categories": [f"c{j}" for j in range(65)]})
    with pytest.raises(ValueError, match="distinct"):
        R.HipIVFFlatIndex({"dimension": 32, "categories": ["a", "a"]})
    index = R.HipFlatIPIndex({"dimension": 32, "categories": ["a", "b", "c"]})
    assert index._item_tags([["a"], [], ["c", "a"], "b"], 4).tolist() == [1, 0, 5, 2]
    assert index._item_tags(np.array([1, 7], np.int64), 2).tolist() == [1, 7]
    with pytest.raises(ValueError, match="bits past"):
        index._item_tags(np.array([8], np.uint64), 1)
    any_of, none_of = index._query_masks(["a", "b"], None, 2)
    assert any_of.tolist() == [3, 3] and none_of.tolist() == [0, 0]
    any_of, none_of = index._query_masks([["a"], ["c"]], "b", 2)
    assert any_of.tolist() == [1, 4] and none_of.tolist() == [2, 2]
    with pytest.raises(ValueError, match="unknown category"):
        index._query_masks(["zz"], None, 1)
    assert R.HipFlatIPIndex({"dimension": 32})._query_masks(None, None, 3) is None


def test_movielens_category_tags():
    import pandas as pd
    from rtrec_amd.data import movielens as ml
    movies = pd.DataFrame({"movie_idx": [0, 1, 2], "genre_action": [1, 0, 0], "genre_comedy": [1, 1, 0],
                           "genre_sci_fi": [0, 1, 0]})
    vocab, tags = ml.movie_category_tags(movies, np.array([2, 1, 0, 9]))
    assert vocab == ["action", "comedy", "sci_fi"]
    assert tags.dtype == np.uint64 and tags.tolist() == [0, 6, 3, 0]
