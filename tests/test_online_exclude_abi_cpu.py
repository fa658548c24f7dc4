"""Host side of rt_flatip_topk_online_lists (the online top-K with exclusion
lists read by the scan): its status codes, returned before any device work
(the pointers below are fakes, never dereferenced), and the ValueErrors of the
Python wrapper, raised before a device is needed. No GPU."""
import ctypes

import pytest
import torch

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_WORKSPACE = 0, -1, -2, -3
BIG = 1 << 40


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    nat.lib()
    return nat


def _sources(nat, *specs):
    """specs: (offsets, items, n_rows, rows) of fake pointers."""
    arr = (nat.ExclusionLists * max(len(specs), 1))()
    for a, (offsets, items, n_rows, rows) in zip(arr, specs):
        a.offsets, a.items, a.n_rows, a.rows = offsets, items, n_rows, rows
    return arr


def _call(nat, lists, n_lists, nq=1, nx=1000, d=128, code=0, k=10, ws_bytes=BIG, q=16, x=16, ws=256, id_offset=0):
    return nat.lib().rt_flatip_topk_online_lists(q, nq, x, nx, d, code, k, lists, n_lists, id_offset, 16, 16, ws,
                                                 ws_bytes, None)


def test_symbol_struct_and_constant(native):
    assert hasattr(native.lib(), "rt_flatip_topk_online_lists")
    assert native.ONLINE_MAX_EXCL_SOURCES == 2
    assert [f for f, _ in native.ExclusionLists._fields_] == ["offsets", "items", "n_rows", "rows"]
    assert ctypes.sizeof(native.ExclusionLists) == 32


def test_list_argument_status_codes(native):
    ok = (16, 16, 4, None)
    assert _call(native, _sources(native, ok), -1) == RT_ERR_INVALID
    assert _call(native, None, 1) == RT_ERR_INVALID
    assert _call(native, _sources(native, (None, 16, 4, None)), 1) == RT_ERR_INVALID       # offsets
    assert _call(native, _sources(native, (16, None, 4, None)), 1) == RT_ERR_INVALID       # items, rows to read
    assert _call(native, _sources(native, (16, 16, -1, None)), 1) == RT_ERR_INVALID        # n_rows
    assert _call(native, _sources(native, ok, (None, 16, 4, None)), 2) == RT_ERR_INVALID   # the second source
    assert _call(native, _sources(native, ok, ok, ok), 3) == RT_ERR_UNSUPPORTED
    # the list refusals come first, and with no device: a call that is invalid
    # both ways reports the lists
    assert _call(native, _sources(native, ok, ok, ok), 3, nq=-1) == RT_ERR_UNSUPPORTED


@pytest.mark.parametrize("n_lists", [0, 1, 2])
def test_every_other_refusal_is_the_old_entrys(native, n_lists):
    """With well-formed lists (or none) the status is rt_flatip_topk_online's."""
    ok = (16, 16, 4, 16)
    lists = _sources(native, ok, (16, None, 0, None))   # an empty CSR needs no items
    f32 = 0

    def both(**kw):
        new = _call(native, lists, n_lists, **kw)
        a = dict(nq=1, nx=1000, d=128, code=f32, k=10, ws_bytes=BIG, q=16, x=16, ws=256, id_offset=0)
        a.update(kw)
        old = native.lib().rt_flatip_topk_online(a["q"], a["nq"], a["x"], a["nx"], a["d"], a["code"], a["k"], None, 0,
                                                 a["id_offset"], 16, 16, a["ws"], a["ws_bytes"], None)
        assert new == old, kw
        return new

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
    assert both(nq=0, ws=None, ws_bytes=0) == RT_OK
    # the size query of the old entry serves the new one: one byte less is refused
    for nq, nx, k in ((1, 1000, 50), (8, 10**6, 128)):
        need = native.lib().rt_flatip_topk_online_workspace_bytes(nq, nx, 128, f32, k)
        assert both(nq=nq, nx=nx, k=k, ws_bytes=need - 1) == RT_ERR_WORKSPACE


def test_wrapper_value_errors(native):
    from rtrec_amd import kernels
    q, x = torch.zeros(2, 128), torch.zeros(100, 128)
    off = torch.zeros(3, dtype=torch.int64)
    it = torch.zeros(4, dtype=torch.int32)
    bits = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        kernels.flatip_topk_online(q, x, 10, exclude_bits=bits, exclude_lists=(off, it))
    with pytest.raises(ValueError, match="sources"):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=[(off, it)] * 3)
    with pytest.raises(ValueError, match="sources"):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=[])
    with pytest.raises(ValueError):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=[(off,)])
    with pytest.raises(TypeError):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=(off, it.to(torch.int64)))
    with pytest.raises(TypeError):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=(off.to(torch.int32), it))
    with pytest.raises(ValueError, match="rows"):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=(off, it, torch.zeros(1, dtype=torch.int64)))
    with pytest.raises(TypeError):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=(off, it, torch.zeros(2, dtype=torch.int32)))
    # well-formed lists of CPU tensors: refused like every CPU tensor, no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.flatip_topk_online(q, x, 10, exclude_lists=(off, it))


def test_host_side_list_helpers():
    """What the searcher and the index do on the host: sort, de-duplicate, drop
    positions outside the corpus and unknown ids."""
    import numpy as np
    from rtrec_amd.serving.retrieval import _exclude_positions, _sorted_positions
    assert _sorted_positions([5, 3, 5, -1, 10, 9], 10).tolist() == [3, 5, 9]
    assert _sorted_positions([], 10).dtype == np.int32
    rev = {"a": 4, "b": 1, "c": 7}
    assert [p.tolist() for p in _exclude_positions(rev, ["c", "zz", "a", "a"], 2)] == [[4, 7], [4, 7]]
    assert [p.tolist() for p in _exclude_positions(rev, [["b"], []], 2)] == [[1], []]
    with pytest.raises(ValueError):
        _exclude_positions(rev, [["b"], [], ["a"]], 2)
