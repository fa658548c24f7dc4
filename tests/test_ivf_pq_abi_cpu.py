"""C-ABI checks of the IVF-PQ entry points that need no GPU (the style of
test_ivf_abi_cpu.py): symbols exported and in the ctypes table, every refusal
returned before any device work (the pointers are dummies), and the workspace
size monotone in nq and M."""
import ctypes

import pytest

from test_ivf_abi_cpu import native  # noqa: F401  (the module fixture: builds and loads the library)

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P16, ODD = ctypes.c_void_p(64), ctypes.c_void_p(72)   # 16-byte aligned / misaligned dummies, never dereferenced
SEARCH = dict(queries=P16, nq=2, d=32, codes=P16, nx=1000, M=8, codebooks=P16, offsets=P16, nlist=16, row_pos=P16,
              probes=P16, bias=None, nprobe=4, max_list_rows=300, k=10, excl=None, words=0, out_s=P16, out_i=P16,
              ws=P16, ws_bytes=0, stream=None)
ENCODE = dict(rows=P16, n=100, d=32, dtype=0, centroids=None, nlist=0, assign=None, codebooks=P16, M=8, codes=P16,
              stream=None)
SHAPES = [dict(M=6), dict(d=272, M=68), dict(d=40, M=12), dict(d=20, M=4), dict(d=144, M=4)]  # M % 4, M <= 64, d % M,
#                                                                                   dsub even, dsub <= 32


def test_symbols_exported_and_listed(native):  # noqa: F811
    for name in ("rt_pq_encode", "rt_ivf_pq_topk", "rt_ivf_pq_topk_workspace_bytes"):
        assert hasattr(native.lib(), name) and name in native.SIGNATURES, name
    assert not native.MISSING


def test_refusals(native):  # noqa: F811
    L = native.lib()
    search = lambda **kw: L.rt_ivf_pq_topk(*{**SEARCH, **kw}.values())  # noqa: E731
    encode = lambda **kw: L.rt_pq_encode(*{**ENCODE, **kw}.values())    # noqa: E731
    W = L.rt_ivf_pq_topk_workspace_bytes(2, 4, 300, 10, 8)
    assert W >= L.rt_ivf_topk_workspace_bytes(2, 4, 300, 10) + 2 * 8 * 1024
    invalid = [{n: None} for n in ("queries", "codes", "codebooks", "offsets", "row_pos", "probes", "out_s", "out_i")]
    invalid += [{n: 0} for n in ("k", "nprobe", "nlist", "d", "M")] + [{n: ODD} for n in ("queries", "codes", "codebooks")]
    invalid += [dict(nx=-1), dict(excl=P16, words=31), dict(ws=ODD, ws_bytes=W)]   # 1000 items need 32 words
    for kw in invalid:
        assert search(**kw) == INVALID, kw
    for kw in SHAPES + [dict(k=129), dict(nprobe=129), dict(nq=65536), dict(nx=2 ** 31 - 1), dict(d=260, M=20)]:
        assert search(**kw) == UNSUPPORTED, kw
    assert search(ws=None) == WORKSPACE and search(ws_bytes=W - 1) == WORKSPACE
    assert search(nq=0) == OK
    invalid = [{n: None} for n in ("rows", "codebooks", "codes")] + [{n: ODD} for n in ("rows", "codebooks")]
    invalid += [dict(centroids=P16, nlist=4), dict(assign=P16), dict(centroids=P16, assign=P16, nlist=0),
                dict(n=-1), dict(d=0), dict(M=0), dict(dtype=5)]
    for kw in invalid:
        assert encode(**kw) == INVALID, kw
    for kw in SHAPES + [dict(d=36, M=4, dtype=1)]:   # 16-bit rows: d % 8
        assert encode(**kw) == UNSUPPORTED, kw
    assert encode(n=0) == OK


def test_workspace_monotone(native):  # noqa: F811
    L = native.lib()
    sizes = [[L.rt_ivf_pq_topk_workspace_bytes(nq, 20, 1500, 100, M) for M in range(4, 65, 4)]
             for nq in (1, 2, 8, 100, 4096)]
    for line in sizes + list(zip(*sizes)):
        assert all(a < b for a, b in zip(line, line[1:]))
    assert L.rt_ivf_pq_topk_workspace_bytes(0, 20, 1500, 100, 16) == 256
    assert L.rt_ivf_pq_topk_workspace_bytes(8, 20, 1500, 100, 6) == 256
