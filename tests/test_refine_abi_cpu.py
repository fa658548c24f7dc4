"""C-ABI checks of rt_refine_topk that need no GPU (the style of test_ivf_pq_abi_cpu.py):
the symbol exported and in the ctypes table, every refusal returned before any device
work (the pointers are dummies, never dereferenced)."""
import ctypes

from test_ivf_abi_cpu import native  # noqa: F401  (the module fixture: builds and loads the library)

OK, INVALID, UNSUPPORTED = 0, -1, -2
P16, ODD8, ODD4 = ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(68)   # aligned to 16 / 8 / 4 only
F32, F16, BF16, SQ8 = 0, 1, 2, 3
ARGS = dict(queries=P16, nq=2, d=32, cand_ids=P16, n_cand=100, store=P16, n_rows=1000, kind=F32, lo=None, step=None,
            k=10, out_s=P16, out_i=P16, stream=None)


def test_symbol_exported_and_listed(native):  # noqa: F811
    assert hasattr(native.lib(), "rt_refine_topk") and "rt_refine_topk" in native.SIGNATURES
    assert not native.MISSING


def test_refusals(native):  # noqa: F811
    refine = lambda **kw: native.lib().rt_refine_topk(*{**ARGS, **kw}.values())  # noqa: E731
    sq8 = dict(kind=SQ8, lo=P16, step=P16)
    invalid = [{n: None} for n in ("queries", "cand_ids", "store", "out_s", "out_i")]
    invalid += [{n: 0} for n in ("k", "n_cand", "d")] + [dict(nq=-1), dict(n_rows=-1), dict(kind=4), dict(kind=-1)]
    invalid += [dict(queries=ODD8), dict(store=ODD8), dict(cand_ids=ODD4), dict(out_i=ODD4), dict(out_s=ctypes.c_void_p(66))]
    invalid += [sq8 | dict(lo=None), sq8 | dict(step=None), sq8 | dict(lo=ODD8), sq8 | dict(step=ODD8)]
    for kw in invalid:
        assert refine(**kw) == INVALID, kw
    unsupported = [dict(n_cand=129, k=10), dict(k=101), dict(nq=65536), dict(d=260), dict(d=30), dict(d=36, kind=F16),
                   dict(d=36, kind=BF16), sq8 | dict(d=40), sq8 | dict(d=272), sq8 | dict(d=8)]
    for kw in unsupported:
        assert refine(**kw) == UNSUPPORTED, kw
    for kw in (dict(nq=0), dict(nq=0, kind=F16), sq8 | dict(nq=0)):
        assert refine(**kw) == OK, kw
    assert refine(nq=0, n_rows=0, store=None) == OK   # an empty store may be NULL
