"""The C ABI of the mutable IVF lists without a GPU: rt_ivf_lists_update,
rt_ivf_lists_update_workspace_bytes, rt_ivf_topk_lens and rt_ivf_topk_lists_lens
are exported and listed in native.SIGNATURES, every refusal the header documents
comes back before any device work (the pointers are dummies), m == 0 is RT_OK,
and the workspace size is monotone."""
import ctypes
import subprocess

import pytest

from conftest import PKG

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
F32, F16 = 0, 1
NEW = ("rt_ivf_lists_update", "rt_ivf_lists_update_workspace_bytes", "rt_ivf_topk_lens", "rt_ivf_topk_lists_lens")


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def test_symbols_are_exported_and_listed(native):
    handle = native.lib()
    for name in NEW:
        assert name in native.SIGNATURES, name
        assert hasattr(handle, name), name
    assert not native.MISSING


def test_workspace_size_is_monotone(native):
    L = native.lib()
    last = 0
    for nlist, m in ((1, 0), (1, 1), (8, 1), (8, 300), (1024, 300), (1024, 1024), (1024, 1 << 20), (65536, 1 << 20)):
        w = L.rt_ivf_lists_update_workspace_bytes(nlist, m)
        assert w >= 4 * (5 * m + 3 * nlist) and w % 256 == 0 and w >= last, (nlist, m, w)
        last = w
    assert L.rt_ivf_lists_update_workspace_bytes(-5, -5) == L.rt_ivf_lists_update_workspace_bytes(0, 0)


def _update(L, **kw):
    """rt_ivf_lists_update on dummy pointers: a valid call except for ``kw``."""
    p = ctypes.c_void_p(64)
    a = dict(rows=p, total_rows=100, d=32, dtype=F32, list_offsets=p, nlist=8, list_len=p, row_pos=p, pos_slot=p,
             assign=p, positions=p, new_list=p, new_rows=p, m=4, status=p, workspace=p, workspace_bytes=1 << 20,
             stream=None)
    a.update(kw)
    return L.rt_ivf_lists_update(*a.values())


def test_update_refusals_before_any_device_work(native):
    L = native.lib()
    for name in ("rows", "list_offsets", "list_len", "row_pos", "pos_slot", "assign", "positions", "new_list",
                 "new_rows", "status"):
        assert _update(L, **{name: None}) == INVALID, name
    assert _update(L, total_rows=-1) == INVALID
    assert _update(L, m=-1) == INVALID
    assert _update(L, nlist=0) == INVALID
    assert _update(L, d=0) == INVALID
    assert _update(L, dtype=7) == INVALID
    assert _update(L, rows=ctypes.c_void_p(72)) == INVALID          # 8 mod 16
    assert _update(L, new_rows=ctypes.c_void_p(68)) == INVALID
    assert _update(L, workspace=ctypes.c_void_p(66)) == INVALID
    assert _update(L, d=30) == UNSUPPORTED                           # f32: d % 4
    assert _update(L, d=36, dtype=F16) == UNSUPPORTED                # f16: d % 8
    assert _update(L, d=260) == UNSUPPORTED                          # d <= 256
    assert _update(L, total_rows=(1 << 31) - 1) == UNSUPPORTED
    assert _update(L, m=(1 << 31) - 1, workspace_bytes=1 << 40) == UNSUPPORTED
    need = L.rt_ivf_lists_update_workspace_bytes(8, 4)
    assert _update(L, workspace_bytes=need - 1) == WORKSPACE
    assert _update(L, workspace=None) == WORKSPACE
    # m == 0: RT_OK without a launch, whatever the other pointers
    assert _update(L, m=0) == OK
    assert _update(L, m=0, positions=None, new_list=None, new_rows=None, status=None, workspace=None,
                   workspace_bytes=0) == OK


def _topk_lens(L, with_lists=False, **kw):
    p = ctypes.c_void_p(64)
    a = dict(queries=p, nq=2, rows=p, nx=100, d=32, dtype=F32, list_offsets=p, nlist=8, list_len=p, n_pos=90,
             row_pos=p, probes=p, nprobe=4, max_list_rows=40, k=10)
    tail = dict(lists=None, n_lists=0) if with_lists else dict(exclude_bits=None, exclude_words=0)
    tail.update(out_scores=p, out_ids=p, workspace=p, workspace_bytes=1 << 24, stream=None)
    a.update(tail)
    a.update(kw)
    fn = L.rt_ivf_topk_lists_lens if with_lists else L.rt_ivf_topk_lens
    return fn(*a.values())


@pytest.mark.parametrize("lists", [False, True])
def test_topk_lens_refusals_before_any_device_work(native, lists):
    L = native.lib()
    assert _topk_lens(L, lists, list_len=None) == INVALID
    assert _topk_lens(L, lists, n_pos=-1) == INVALID
    assert _topk_lens(L, lists, n_pos=(1 << 31) - 1) == UNSUPPORTED
    assert _topk_lens(L, lists, queries=None) == INVALID
    assert _topk_lens(L, lists, nprobe=0) == INVALID
    assert _topk_lens(L, lists, k=129) == UNSUPPORTED
    assert _topk_lens(L, lists, d=30) == UNSUPPORTED
    assert _topk_lens(L, lists, workspace_bytes=16) == WORKSPACE
    assert _topk_lens(L, lists, nq=0) == OK
    if lists:
        assert _topk_lens(L, lists, n_lists=-1) == INVALID
        assert _topk_lens(L, lists, n_lists=3, lists=(native.ExclusionLists * 3)()) == UNSUPPORTED
    else:
        # the bitmap is as wide as the positions, not as the stored rows: ceil(90 / 32) = 3 words
        p = ctypes.c_void_p(64)
        assert _topk_lens(L, lists, exclude_bits=p, exclude_words=2) == INVALID
        assert _topk_lens(L, lists, exclude_bits=p, exclude_words=3, workspace_bytes=16) == WORKSPACE
