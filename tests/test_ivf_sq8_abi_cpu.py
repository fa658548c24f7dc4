"""C-ABI checks of the IVF-SQ8 entry points that need no GPU (the style of
test_ivf_pq_abi_cpu.py): symbols exported and in the ctypes table, every refusal
returned before any device work (the pointers are dummies), and the workspace
size monotone in nq and d."""
import ctypes

from test_ivf_abi_cpu import native  # noqa: F401  (the module fixture: builds and loads the library)

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P16, ODD = ctypes.c_void_p(64), ctypes.c_void_p(72)   # 16-byte aligned / misaligned dummies, never dereferenced
SEARCH = dict(queries=P16, nq=2, d=32, codes=P16, nx=1000, lo=P16, step=P16, offsets=P16, nlist=16, row_pos=P16,
              probes=P16, bias=None, nprobe=4, max_list_rows=300, k=10, excl=None, words=0, out_s=P16, out_i=P16,
              ws=P16, ws_bytes=0, stream=None)
ENCODE = dict(rows=P16, n=100, d=32, dtype=0, centroids=None, nlist=0, assign=None, lo=P16, inv_step=P16, codes=P16,
              stream=None)
SHAPES = [dict(d=8), dict(d=24), dict(d=272), dict(d=260)]   # below 16, d % 16, above 256


def test_symbols_exported_and_listed(native):  # noqa: F811
    for name in ("rt_sq8_encode", "rt_ivf_sq8_topk", "rt_ivf_sq8_topk_workspace_bytes"):
        assert hasattr(native.lib(), name) and name in native.SIGNATURES, name
    assert not native.MISSING


def test_refusals(native):  # noqa: F811
    L = native.lib()
    search = lambda **kw: L.rt_ivf_sq8_topk(*{**SEARCH, **kw}.values())  # noqa: E731
    encode = lambda **kw: L.rt_sq8_encode(*{**ENCODE, **kw}.values())    # noqa: E731
    W = L.rt_ivf_sq8_topk_workspace_bytes(2, 4, 300, 10, 32)
    assert W >= L.rt_ivf_topk_workspace_bytes(2, 4, 300, 10) + 2 * (32 + 4) * 4
    invalid = [{n: None} for n in ("queries", "codes", "lo", "step", "offsets", "row_pos", "probes", "out_s", "out_i")]
    invalid += [{n: 0} for n in ("k", "nprobe", "nlist", "d")] + [{n: ODD} for n in ("queries", "codes", "lo", "step")]
    invalid += [dict(nx=-1), dict(bias=ctypes.c_void_p(66)), dict(excl=P16, words=31), dict(ws=ODD, ws_bytes=W)]
    for kw in invalid:
        assert search(**kw) == INVALID, kw
    for kw in SHAPES + [dict(k=129), dict(nprobe=129), dict(nq=65536), dict(nx=2 ** 31 - 1)]:
        assert search(**kw) == UNSUPPORTED, kw
    assert search(ws=None) == WORKSPACE and search(ws_bytes=W - 1) == WORKSPACE
    assert search(nq=0) == OK
    invalid = [{n: None} for n in ("rows", "lo", "inv_step", "codes")]
    invalid += [{n: ODD} for n in ("rows", "lo", "inv_step", "codes")]
    invalid += [dict(centroids=P16, nlist=4), dict(assign=P16), dict(centroids=P16, assign=P16, nlist=0),
                dict(centroids=ODD, assign=P16, nlist=4), dict(n=-1), dict(d=0), dict(dtype=5)]
    for kw in invalid:
        assert encode(**kw) == INVALID, kw
    for kw in SHAPES + [dict(n=2 ** 40, d=256)]:
        assert encode(**kw) == UNSUPPORTED, kw
    assert encode(n=0) == OK


def test_workspace_monotone(native):  # noqa: F811
    L = native.lib()
    sizes = [[L.rt_ivf_sq8_topk_workspace_bytes(nq, 20, 1500, 100, d) for d in range(16, 257, 16)]
             for nq in (1, 2, 8, 100, 4096, 65535)]
    for line in sizes + list(zip(*sizes)):
        assert all(a < b for a, b in zip(line, line[1:]))
    for kw in (dict(nq=0), dict(nq=65536), dict(d=24), dict(d=272), dict(k=129), dict(k=0), dict(nprobe=129)):
        args = {**dict(nq=8, nprobe=20, mlr=1500, k=100, d=128), **kw}
        assert L.rt_ivf_sq8_topk_workspace_bytes(*args.values()) == 256, kw
