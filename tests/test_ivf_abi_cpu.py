"""C-ABI checks of the IVF entry points that need no GPU: the symbols are
exported and in the ctypes table, every refusal comes back as the documented
status before any device work (the pointers are dummies), and the host-only
plan keeps its invariants."""
import ctypes
import subprocess

import pytest

from conftest import PKG

IVF_SYMBOLS = ["rt_ivf_topk", "rt_ivf_topk_plan", "rt_ivf_topk_workspace_bytes", "rt_ivf_topk_tuning",
               "rt_segment_mean_f32"]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
F32, F16, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def test_symbols_exported_and_listed(native):
    handle = native.lib()
    for name in IVF_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in native.SIGNATURES, name
    assert not native.MISSING


P16 = ctypes.c_void_p(64)   # a non-NULL, 16-byte aligned dummy: never dereferenced by a refusal


def _ivf(L, **kw):
    a = dict(queries=P16, nq=2, rows=P16, nx=1000, d=32, dtype=F32, offsets=P16, nlist=16, row_pos=P16, probes=P16,
             nprobe=4, max_list_rows=300, k=10, excl=None, words=0, out_s=P16, out_i=P16, ws=P16, ws_bytes=0)
    a.update(kw)
    return L.rt_ivf_topk(a["queries"], a["nq"], a["rows"], a["nx"], a["d"], a["dtype"], a["offsets"], a["nlist"],
                         a["row_pos"], a["probes"], a["nprobe"], a["max_list_rows"], a["k"], a["excl"], a["words"],
                         a["out_s"], a["out_i"], a["ws"], a["ws_bytes"], None)


def test_ivf_topk_refusals(native):
    L = native.lib()
    for name in ("queries", "rows", "offsets", "row_pos", "probes", "out_s", "out_i"):
        assert _ivf(L, **{name: None}) == INVALID, name
    assert _ivf(L, k=0) == INVALID
    assert _ivf(L, k=129) == UNSUPPORTED
    assert _ivf(L, nprobe=0) == INVALID
    assert _ivf(L, nprobe=129) == UNSUPPORTED
    assert _ivf(L, dtype=3) == INVALID
    assert _ivf(L, d=0) == INVALID
    assert _ivf(L, d=260) == UNSUPPORTED            # d <= 256
    assert _ivf(L, d=6) == UNSUPPORTED              # f32: d % 4
    assert _ivf(L, d=12, dtype=F16) == UNSUPPORTED  # 16-bit: d % 8
    assert _ivf(L, d=12, dtype=BF16) == UNSUPPORTED
    assert _ivf(L, nq=65536) == UNSUPPORTED
    assert _ivf(L, queries=ctypes.c_void_p(72)) == INVALID   # misaligned
    assert _ivf(L, excl=P16, words=31) == INVALID            # 1000 items need 32 words
    # everything valid but the workspace: NULL, then one byte short
    assert _ivf(L, ws=None) == WORKSPACE
    W = L.rt_ivf_topk_workspace_bytes(2, 4, 300, 10)
    assert W > 256
    assert _ivf(L, ws_bytes=W - 1) == WORKSPACE
    assert _ivf(L, nq=0) == OK
    with pytest.raises(native.RTError):
        native.call("rt_ivf_topk", None, 1, None, 0, 32, 0, None, 1, None, None, 1, 0, 1, None, 0, None, None, None,
                    0, None)


def test_segment_mean_refusals(native):
    L = native.lib()

    def call(rows=P16, n=100, d=32, dtype=F32, offsets=P16, n_seg=4, prev=P16, normalize=0, out=P16):
        return L.rt_segment_mean_f32(rows, n, d, dtype, offsets, n_seg, prev, normalize, out, None)

    for name in ("rows", "offsets", "prev", "out"):
        assert call(**{name: None}) == INVALID, name
    assert call(dtype=7) == INVALID
    assert call(d=0) == INVALID
    assert call(n=-1) == INVALID
    assert call(d=260) == UNSUPPORTED
    assert call(d=6) == UNSUPPORTED
    assert call(d=12, dtype=F16) == UNSUPPORTED
    assert call(rows=ctypes.c_void_p(72)) == INVALID
    assert call(n_seg=0) == OK


@pytest.mark.parametrize("nq", [1, 8, 100])
@pytest.mark.parametrize("nprobe", [1, 20, 128])
@pytest.mark.parametrize("max_list_rows", [0, 1, 255, 256, 257, 5000])
def test_plan_invariants(native, nq, nprobe, max_list_rows):
    L = native.lib()
    out = (ctypes.c_int64 * 3)()
    assert L.rt_ivf_topk_plan(nq, nprobe, max_list_rows, ctypes.cast(out, ctypes.c_void_p)) == OK
    chunks, rows_per_chunk, blocks = out[0], out[1], out[2]
    assert chunks >= 1 and rows_per_chunk >= 1
    assert chunks * rows_per_chunk >= max_list_rows
    assert blocks == nq * nprobe * chunks
    for k in (1, 10, 128):
        assert L.rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k) >= nprobe * chunks * nq * k * 8


def test_plan_refusals(native):
    L = native.lib()
    out = (ctypes.c_int64 * 3)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert L.rt_ivf_topk_plan(1, 20, 100, None) == INVALID
    assert L.rt_ivf_topk_plan(0, 20, 100, p) == INVALID
    assert L.rt_ivf_topk_plan(1, 129, 100, p) == UNSUPPORTED
    assert L.rt_ivf_topk_workspace_bytes(1, 129, 100, 10) == 256
