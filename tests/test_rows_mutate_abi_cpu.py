"""rt_scatter_rows / rt_rows_compact at the C-ABI boundary, without a GPU:
every argument error comes back as RT_ERR_INVALID before any device work (the
pointers are dummies that are never dereferenced), the workspace query is
host arithmetic, empty calls are RT_OK with null row pointers, and the torch
wrappers refuse CPU tensors."""
import ctypes
import subprocess

import pytest
import torch

from conftest import PKG

RT_OK, RT_ERR_INVALID = 0, -1
SRC, DST, BITS, WS, OUT = (ctypes.c_void_p(a) for a in (0x10000000, 0x90000000, 0x20, 0x40, 0x80))


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def _compact(L, src=SRC, n_rows=1000, row_bytes=256, bits=BITS, words=None, dst=DST, dst_rows=None, n_kept=OUT,
             ws=WS, ws_bytes=None):
    words = -(-n_rows // 32) if words is None else words
    dst_rows = n_rows if dst_rows is None else dst_rows
    ws_bytes = L.rt_rows_compact_workspace_bytes(n_rows) if ws_bytes is None else ws_bytes
    return L.rt_rows_compact(src, n_rows, row_bytes, bits, words, dst, dst_rows, n_kept, ws, ws_bytes, None)


def test_scatter_argument_errors(native):
    L = native.lib()

    def scatter(src=SRC, n=4, row_bytes=256, pos=BITS, dst=DST, dst_rows=1000):
        return L.rt_scatter_rows(src, n, row_bytes, pos, dst, dst_rows, None, None)

    assert scatter(src=ctypes.c_void_p(0x10008)) == RT_ERR_INVALID      # src not 16-byte aligned
    assert scatter(dst=ctypes.c_void_p(0x900004)) == RT_ERR_INVALID     # dst not 16-byte aligned
    for row_bytes in (0, 8, 24, 250, -16):
        assert scatter(row_bytes=row_bytes) == RT_ERR_INVALID, row_bytes
    assert scatter(n=-1) == RT_ERR_INVALID
    assert scatter(src=None) == RT_ERR_INVALID
    assert scatter(pos=None) == RT_ERR_INVALID
    assert scatter(dst=None) == RT_ERR_INVALID
    # nothing to do: RT_OK without a launch, null row pointers
    assert scatter(src=None, n=0, pos=None, dst=None, dst_rows=0) == RT_OK
    assert scatter(src=None, n=0, pos=None, dst=None) == RT_OK
    with pytest.raises(native.RTError):
        native.call("rt_scatter_rows", SRC, 4, 250, BITS, DST, 1000, None, None)


def test_compact_argument_errors(native):
    L = native.lib()
    assert _compact(L, src=ctypes.c_void_p(0x10004)) == RT_ERR_INVALID  # misaligned rows
    assert _compact(L, dst=ctypes.c_void_p(0x900008)) == RT_ERR_INVALID
    for row_bytes in (0, 4, 40, 1036, -256):                            # not a multiple of 16
        assert _compact(L, row_bytes=row_bytes) == RT_ERR_INVALID, row_bytes
    assert _compact(L, n_rows=-1, words=0, dst_rows=0, ws_bytes=256) == RT_ERR_INVALID
    # overlap: dst inside src, src inside dst, equal, dst's spare rows reaching into src
    n, rb = 1000, 256
    assert _compact(L, dst=SRC) == RT_ERR_INVALID
    assert _compact(L, dst=ctypes.c_void_p(SRC.value + (n - 1) * rb)) == RT_ERR_INVALID
    assert _compact(L, dst=ctypes.c_void_p(SRC.value - (n - 1) * rb)) == RT_ERR_INVALID
    assert _compact(L, dst=ctypes.c_void_p(SRC.value - 2 * n * rb), dst_rows=2 * n + 1) == RT_ERR_INVALID
    assert _compact(L, n_rows=n, dst_rows=n - 1) == RT_ERR_INVALID      # dst_rows < n_rows
    for n_rows in (1, 32, 33, 1000, 2049):                              # short bitmap
        assert _compact(L, n_rows=n_rows, words=-(-n_rows // 32) - 1) == RT_ERR_INVALID, n_rows
    for n_rows in (1, 2048, 2049, 10**6):                               # one byte short of the query's answer
        W = L.rt_rows_compact_workspace_bytes(n_rows)
        assert _compact(L, n_rows=n_rows, ws_bytes=W - 1) == RT_ERR_INVALID, n_rows
    assert _compact(L, ws=None) == RT_ERR_INVALID
    assert _compact(L, ws=ctypes.c_void_p(0x44)) == RT_ERR_INVALID      # workspace not 8-byte aligned
    assert _compact(L, n_kept=None) == RT_ERR_INVALID
    assert _compact(L, bits=None) == RT_ERR_INVALID
    with pytest.raises(native.RTError):
        native.call("rt_rows_compact", SRC, 10, 256, BITS, 1, DST, 9, OUT, WS, 256, None)


def test_compact_workspace_query_is_monotone(native):
    L = native.lib()
    sizes = [L.rt_rows_compact_workspace_bytes(n) for n in
             (0, 1, 31, 32, 2047, 2048, 2049, 65536, 10**6, 10**6 + 1, 10**8, 2**33)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert sizes[-1] >= (2**33 // 2048 + 1) * 8                         # one int64 per 2,048-row segment, plus one
    assert L.rt_rows_compact_workspace_bytes(-5) == sizes[0]


def test_empty_calls_are_ok_with_null_row_pointers(native):
    L = native.lib()
    W = L.rt_rows_compact_workspace_bytes(0)
    # n_rows == 0 and nowhere to report the count: host-only, nothing is touched
    assert L.rt_rows_compact(None, 0, 256, None, 0, None, 0, None, None, W, None) == RT_OK
    assert L.rt_rows_compact(None, 0, 1040, None, 0, None, 100, None, None, W, None) == RT_OK
    assert L.rt_scatter_rows(None, 0, 16, None, None, 0, None, None) == RT_OK


def test_wrappers_refuse_cpu_tensors_and_bad_rows(native):
    from rtrec_amd import kernels
    t = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.scatter_rows(t, torch.zeros(8, dtype=torch.int64), t.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.rows_compact(t, torch.zeros(1, dtype=torch.int32), t.clone())


def test_non_mutable_index_is_the_default_and_only_warns(native, caplog):
    """``mutable`` defaults to off: update / remove log the reference's warning and
    touch nothing (no device is needed to say so)."""
    import logging
    from rtrec_amd.serving import HipFlatIPIndex
    index = HipFlatIPIndex({"dimension": 32, "metric": "cosine"})
    assert index.mutable is False and HipFlatIPIndex({"dimension": 32, "mutable": True}).mutable is True
    with caplog.at_level(logging.WARNING, logger="rtrec_amd.retrieval"):
        assert index.update(torch.zeros(1, 32), ["a"]) is None
        assert index.remove(["a"]) is None
    text = caplog.text
    assert "Flat index doesn't support direct updates. Consider periodic rebuilds." in text
    assert "Flat index doesn't support removal. Consider periodic rebuilds." in text
    assert index.index is None and index.current_size == 0 and index._generation == 0
