"""C-ABI checks of rt_ivf_sq8_topk_batch (csrc/ivf_sq8_batch.hip) that need no GPU, in the
style of test_ivf_sq8_abi_cpu.py: symbols exported and in the ctypes table, every refusal of
rt_ivf_sq8_topk and of rt_ivf_topk_batch returned before any device work (the pointers are
dummies), and the workspace formula, monotone in nq and d."""
import ctypes

from test_ivf_abi_cpu import native  # noqa: F401  (the module fixture: builds and loads the library)

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P16, ODD = ctypes.c_void_p(64), ctypes.c_void_p(72)   # 16-byte aligned / misaligned dummies, never dereferenced
SEARCH = dict(queries=P16, nq=40, d=32, codes=P16, nx=1000, lo=P16, step=P16, offsets=P16, nlist=16, row_pos=P16,
              probes=P16, bias=None, nprobe=4, max_list_rows=300, k=10, excl=None, words=0, out_s=P16, out_i=P16,
              ws=P16, ws_bytes=0, stream=None)
SHAPES = [dict(d=8), dict(d=24), dict(d=272), dict(d=260)]   # below 16, d % 16, above 256


def test_symbols_exported_and_listed(native):  # noqa: F811
    for name in ("rt_ivf_sq8_topk_batch", "rt_ivf_sq8_topk_batch_workspace_bytes"):
        assert hasattr(native.lib(), name) and name in native.SIGNATURES, name
    assert not native.MISSING


def test_refusals(native):  # noqa: F811
    L = native.lib()
    search = lambda **kw: L.rt_ivf_sq8_topk_batch(*{**SEARCH, **kw}.values())  # noqa: E731
    W = L.rt_ivf_sq8_topk_batch_workspace_bytes(40, 4, 16, 300, 10, 32)
    invalid = [{n: None} for n in ("queries", "codes", "lo", "step", "offsets", "row_pos", "probes", "out_s", "out_i")]
    invalid += [{n: 0} for n in ("k", "nprobe", "nlist", "d")] + [{n: ODD} for n in ("queries", "codes", "lo", "step")]
    invalid += [dict(nq=-1), dict(nx=-1), dict(max_list_rows=-1), dict(bias=ctypes.c_void_p(66)),
                dict(excl=P16, words=31), dict(ws=ODD, ws_bytes=W)]
    for kw in invalid:
        assert search(**kw) == INVALID, kw
    limits = [dict(k=129), dict(nprobe=129), dict(nx=2 ** 31 - 1), dict(nq=2 ** 31 // 4), dict(nlist=2 ** 31 - 1),
              dict(max_list_rows=2 ** 32 - 1)]
    for kw in SHAPES + limits:
        assert search(**kw) == UNSUPPORTED, kw
    assert search(ws=None, ws_bytes=W) == WORKSPACE and search(ws_bytes=W - 1) == WORKSPACE
    assert search(nq=0) == OK
    assert search(nq=0, queries=None, probes=None, ws=None) == OK   # nothing is read


def test_workspace_formula_and_monotone(native):  # noqa: F811
    L = native.lib()
    size, tables = L.rt_ivf_sq8_topk_batch_workspace_bytes, L.rt_ivf_topk_batch_workspace_bytes
    for nq, nprobe, d in ((1, 1, 16), (40, 4, 32), (4096, 20, 128), (70, 7, 256)):
        assert tables(nq, nprobe, 1024, 1500, 100) % 256 == 0
        assert size(nq, nprobe, 1024, 1500, 100, d) == (tables(nq, nprobe, 1024, 1500, 100)
                                                        + nq * (d + (nprobe + 3) // 4 * 4) * 4)
    sizes = [[size(nq, 20, 1024, 1500, 100, d) for d in range(16, 257, 16)] for nq in (1, 2, 8, 100, 4096, 100000)]
    for line in sizes + list(zip(*sizes)):
        assert all(a < b for a, b in zip(line, line[1:]))
    for kw in (dict(nq=0), dict(nq=2 ** 31 // 20), dict(d=24), dict(d=272), dict(k=129), dict(k=0), dict(nprobe=129),
               dict(nlist=0), dict(mlr=-1)):
        args = {**dict(nq=8, nprobe=20, nlist=1024, mlr=1500, k=100, d=128), **kw}
        assert size(*args.values()) == 256, kw
