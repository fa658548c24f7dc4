"""rt_ivf_topk_wide without a GPU: exported and in the ctypes table, every refusal is
the documented status before any launch (dummy pointers, no device), and the
workspace size is monotone in k and 256 for a refused shape."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P16 = ctypes.c_void_p(64)   # non-NULL, 16-byte aligned: never dereferenced by a refusal


@pytest.fixture(scope="module")
def L():
    from rtrec_amd import native as nat
    lib = nat.lib()
    assert {"rt_ivf_topk_wide", "rt_ivf_topk_wide_workspace_bytes"} <= set(nat.SIGNATURES) and not nat.MISSING
    return lib


def _wide(L, **kw):
    a = dict(queries=P16, nq=2, rows=P16, nx=1000, d=32, dtype=0, offsets=P16, nlist=16, list_len=None, n_pos=1000,
             row_pos=P16, probes=P16, nprobe=4, max_list_rows=300, k=300, excl=None, words=0, out_s=P16, out_i=P16,
             ws=P16, ws_bytes=0, stream=None)
    a.update(kw)
    return L.rt_ivf_topk_wide(*a.values())


def test_refusals(L):
    for name in ("queries", "rows", "offsets", "row_pos", "probes", "out_s", "out_i"):
        assert _wide(L, **{name: None}) == INVALID, name
    for kw, want in [(dict(k=0), INVALID), (dict(k=1025), UNSUPPORTED), (dict(nprobe=0), INVALID),
                     (dict(nprobe=129), UNSUPPORTED), (dict(nq=65536), UNSUPPORTED), (dict(nq=-1), INVALID),
                     (dict(n_pos=-1), INVALID), (dict(dtype=3), INVALID), (dict(d=12, dtype=1), UNSUPPORTED),
                     (dict(queries=ctypes.c_void_p(72)), INVALID), (dict(excl=P16, words=31), INVALID),
                     (dict(ws=None), WORKSPACE), (dict(nq=0, ws=None), OK)]:
        assert _wide(L, **kw) == want, kw
    W = L.rt_ivf_topk_wide_workspace_bytes(2, 4, 300, 300)
    assert W > 256 and _wide(L, ws_bytes=W - 1) == WORKSPACE
    assert _wide(L, ws_bytes=W - 1, list_len=P16) == WORKSPACE   # list_len is optional, not a refusal


@pytest.mark.parametrize("nq,nprobe,max_list_rows", [(1, 20, 1500), (8, 1, 0), (100, 128, 5000), (3, 8, 255)])
def test_workspace_bytes(L, nq, nprobe, max_list_rows):
    out = (ctypes.c_int64 * 3)()
    assert L.rt_ivf_topk_plan(nq, nprobe, max_list_rows, ctypes.cast(out, ctypes.c_void_p)) == OK
    ws, prev = L.rt_ivf_topk_wide_workspace_bytes, 0
    for k in (1, 128, 129, 256, 257, 1000, 1024):   # a count and min(k, rows per chunk) keys per scan block
        W = ws(nq, nprobe, max_list_rows, k)
        assert W >= prev and W >= out[2] * (min(k, out[1]) + 1) * 8
        prev = W
    assert [ws(nq, nprobe, max_list_rows, 0), ws(nq, nprobe, max_list_rows, 1025), ws(0, nprobe, max_list_rows, 10),
            ws(nq, 129, max_list_rows, 10), ws(65536, nprobe, max_list_rows, 10)] == [256] * 5
