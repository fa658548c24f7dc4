"""Host side of rt_ivf_topk_lists (the probed-list scan with exclusion lists)
that needs no GPU: the symbol is exported and in the ctypes table, every
refusal comes back as the documented status before any device work (the
pointers are dummies), and kernels.ivf_topk refuses malformed exclude_lists
on the host."""
import ctypes
import subprocess

import pytest
import torch

from conftest import PKG

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
F32, F16, BF16 = 0, 1, 2
P16 = ctypes.c_void_p(64)   # a non-NULL, 16-byte aligned dummy: never dereferenced by a refusal
PTR = 64


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def _sources(native, *specs):
    """An RtExclusionLists array from (offsets, items, n_rows, rows) pointer tuples."""
    arr = (native.ExclusionLists * max(len(specs), 1))()
    for a, (offsets, items, n_rows, rows) in zip(arr, specs):
        a.offsets, a.items, a.n_rows, a.rows = offsets, items, n_rows, rows
    return arr


def _ivf(native, lists, n_lists, **kw):
    a = dict(queries=P16, nq=2, rows=P16, nx=1000, d=32, dtype=F32, offsets=P16, nlist=16, row_pos=P16, probes=P16,
             nprobe=4, max_list_rows=300, k=10, out_s=P16, out_i=P16, ws=P16, ws_bytes=0)
    a.update(kw)
    return native.lib().rt_ivf_topk_lists(a["queries"], a["nq"], a["rows"], a["nx"], a["d"], a["dtype"], a["offsets"],
                                          a["nlist"], a["row_pos"], a["probes"], a["nprobe"], a["max_list_rows"],
                                          a["k"], lists, n_lists, a["out_s"], a["out_i"], a["ws"], a["ws_bytes"],
                                          None)


def test_symbol_exported_and_listed(native):
    assert hasattr(native.lib(), "rt_ivf_topk_lists")
    assert "rt_ivf_topk_lists" in native.SIGNATURES
    assert not native.MISSING


def test_list_refusals(native):
    ok = (PTR, PTR, 2, None)
    one = _sources(native, ok)
    assert _ivf(native, one, -1) == INVALID
    assert _ivf(native, None, 1) == INVALID
    assert _ivf(native, _sources(native, (None, PTR, 2, None)), 1) == INVALID      # offsets == NULL
    assert _ivf(native, _sources(native, (PTR, PTR, -1, None)), 1) == INVALID      # n_rows < 0
    assert _ivf(native, _sources(native, (PTR, None, 2, None)), 1) == INVALID      # items == NULL, n_rows > 0
    assert _ivf(native, _sources(native, ok, (PTR, None, 1, PTR)), 2) == INVALID   # the second source is checked too
    assert _ivf(native, _sources(native, ok, ok, ok), 3) == UNSUPPORTED
    # the list checks come first: three sources with an otherwise invalid call
    assert _ivf(native, _sources(native, ok, ok, ok), 3, k=0) == UNSUPPORTED
    # a source without rows may have no items
    assert _ivf(native, _sources(native, (PTR, None, 0, None)), 1, nq=0) == OK


@pytest.mark.parametrize("n_lists", [0, 1, 2])
def test_refusals_of_rt_ivf_topk(native, n_lists):
    lists = _sources(native, (PTR, PTR, 2, None), (PTR, PTR, 5, PTR))

    def call(**kw):
        return _ivf(native, lists, n_lists, **kw)

    for name in ("queries", "rows", "offsets", "row_pos", "probes", "out_s", "out_i"):
        assert call(**{name: None}) == INVALID, name
    assert call(k=0) == INVALID
    assert call(k=129) == UNSUPPORTED
    assert call(nprobe=0) == INVALID
    assert call(nprobe=129) == UNSUPPORTED
    assert call(nlist=0) == INVALID
    assert call(nx=-1) == INVALID
    assert call(max_list_rows=-1) == INVALID
    assert call(dtype=3) == INVALID
    assert call(d=0) == INVALID
    assert call(d=260) == UNSUPPORTED
    assert call(d=6) == UNSUPPORTED
    assert call(d=12, dtype=F16) == UNSUPPORTED
    assert call(d=12, dtype=BF16) == UNSUPPORTED
    assert call(nq=65536) == UNSUPPORTED
    assert call(nx=2 ** 31 - 1) == UNSUPPORTED
    assert call(queries=ctypes.c_void_p(72)) == INVALID   # misaligned
    assert call(ws=None) == WORKSPACE
    W = native.lib().rt_ivf_topk_workspace_bytes(2, 4, 300, 10)
    assert call(ws_bytes=W - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(68), ws_bytes=W) == INVALID   # workspace: 8-byte aligned
    assert call(nq=0) == OK


def _cpu_operands(nq=2):
    q = torch.zeros((nq, 4))
    rows = torch.zeros((16, 4))
    offsets = torch.tensor([0, 16], dtype=torch.int64)
    row_pos = torch.arange(16, dtype=torch.int32)
    probes = torch.zeros((nq, 1), dtype=torch.int64)
    return q, rows, offsets, row_pos, probes


def test_wrapper_refuses_on_the_host(native):
    """ValueError / TypeError for malformed exclusions before a device is needed:
    every operand here is a CPU tensor, which the device check that follows
    would refuse with another error."""
    from rtrec_amd import kernels
    q, rows, offsets, row_pos, probes = _cpu_operands()
    src = (torch.tensor([0, 1, 2], dtype=torch.int64), torch.tensor([3, 5], dtype=torch.int32))
    bits = torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1, exclude_bits=bits, exclude_lists=src)
    with pytest.raises(ValueError, match="3 sources"):
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1, exclude_lists=[src, src, src])
    with pytest.raises(ValueError):
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1, exclude_lists=[])
    with pytest.raises(TypeError):
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1,
                         exclude_lists=(src[0], src[1].to(torch.int64)))
    with pytest.raises(ValueError, match="rows"):   # rows shorter than the queries
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1,
                         exclude_lists=(src[0], src[1], torch.zeros(1, dtype=torch.int64)))
    # well-formed lists pass the host checks and reach the device check: no CPU fallback
    with pytest.raises(RuntimeError):
        kernels.ivf_topk(q, rows, offsets, row_pos, probes, 16, 1, exclude_lists=src)
