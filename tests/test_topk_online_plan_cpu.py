"""Host side of the online (small-batch) Flat-IP top-K: the row-sized plan of
rt_flatip_topk_online_plan, the status codes of rt_flatip_topk_online and the
size query. No GPU: the entry points validate before any device work, the
plan does none at all."""
import ctypes
import itertools

import pytest
import torch

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_WORKSPACE = 0, -1, -2, -3
MAX_BLOCKS = 512  # 2 per CU

NX = (0, 1, 63, 1_000, 4_097, 131_072, 10**6, 10**7)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DIMS = (8, 128, 256)


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    nat.lib()
    return nat


def _plan(nat, nq, nx, d, code, k):
    out = (ctypes.c_int64 * 2)(-1, -1)
    rc = nat.lib().rt_flatip_topk_online_plan(nq, nx, d, code, k, ctypes.cast(out, ctypes.c_void_p))
    return rc, int(out[0]), int(out[1])


@pytest.mark.parametrize("nx", NX)
def test_plan_invariants(native, nx):
    """1 <= blocks <= 512; the blocks cover the corpus; no block is empty (an
    empty corpus cannot satisfy that with its one block: there the plan is one
    block, which the scan never launches); the plan is a function of its inputs."""
    for dtype, d, (nq, k) in itertools.product(DTYPES, DIMS, ((1, 1), (1, 100), (8, 128))):
        code = native.dtype_code(dtype)
        rc, blocks, rpb = _plan(native, nq, nx, d, code, k)
        assert rc == RT_OK, (nx, dtype, d)
        assert 1 <= blocks <= MAX_BLOCKS
        assert rpb >= 1
        assert blocks * rpb >= nx
        if nx > 0:
            assert (blocks - 1) * rpb < nx
        else:
            assert blocks == 1
        assert _plan(native, nq, nx, d, code, k) == (rc, blocks, rpb)


def test_plan_fills_the_chip_on_a_large_corpus(native):
    rc, blocks, rpb = _plan(native, 1, 10**6, 128, native.RT_F16, 100)
    assert rc == RT_OK and blocks == MAX_BLOCKS and rpb == -(-10**6 // MAX_BLOCKS)


def test_plan_wrapper_matches_the_abi(native):
    from rtrec_amd import kernels
    for nx in NX:
        rc, blocks, rpb = _plan(native, 3, nx, 128, native.RT_F32, 50)
        assert kernels.flatip_topk_online_plan(3, nx, 128, torch.float32, 50) == (blocks, rpb)


def test_plan_status_codes(native):
    f32 = native.RT_F32
    assert _plan(native, 9, 1000, 128, f32, 10)[0] == RT_ERR_UNSUPPORTED
    assert _plan(native, 1, 1000, 128, f32, 129)[0] == RT_ERR_UNSUPPORTED
    assert _plan(native, 1, 1000, 130, f32, 10)[0] == RT_ERR_UNSUPPORTED     # d % 4
    assert _plan(native, 1, 1000, 132, native.RT_F16, 10)[0] == RT_ERR_UNSUPPORTED  # d % 8
    assert _plan(native, 1, 1000, 260, f32, 10)[0] == RT_ERR_UNSUPPORTED
    assert _plan(native, 0, 1000, 128, f32, 10)[0] == RT_ERR_INVALID
    assert _plan(native, 1, -1, 128, f32, 10)[0] == RT_ERR_INVALID
    assert _plan(native, 1, 1000, 128, 7, 10)[0] == RT_ERR_INVALID
    assert native.lib().rt_flatip_topk_online_plan(1, 1000, 128, f32, 10, None) == RT_ERR_INVALID


def _call(nat, nq, nx, d, code, k, ws_bytes, q=16, x=16, ws=256, words=0, excl=None, id_offset=0):
    """rt_flatip_topk_online with fake (aligned, never dereferenced) pointers:
    every case below is refused before any device work."""
    return nat.lib().rt_flatip_topk_online(q, nq, x, nx, d, code, k, excl, words, id_offset, 16, 16, ws, ws_bytes, None)


def test_entry_status_codes(native):
    f32 = native.RT_F32
    big = 1 << 40
    assert _call(native, 9, 1000, 128, f32, 10, big) == RT_ERR_UNSUPPORTED
    assert _call(native, 1, 1000, 128, f32, 129, big) == RT_ERR_UNSUPPORTED
    assert _call(native, 1, 1000, 130, f32, 10, big) == RT_ERR_UNSUPPORTED
    assert _call(native, 1, 1 << 32, 128, f32, 10, big) == RT_ERR_UNSUPPORTED
    assert _call(native, 1, 1000, 128, f32, 10, big, id_offset=-1) == RT_ERR_UNSUPPORTED
    assert _call(native, -1, 1000, 128, f32, 10, big) == RT_ERR_INVALID
    assert _call(native, 1, 1000, 128, f32, 0, big) == RT_ERR_INVALID
    assert _call(native, 1, 1000, 128, 5, 10, big) == RT_ERR_INVALID
    assert _call(native, 1, 1000, 128, f32, 10, big, q=None) == RT_ERR_INVALID
    assert _call(native, 1, 1000, 128, f32, 10, big, x=None) == RT_ERR_INVALID
    assert _call(native, 1, 1000, 128, f32, 10, big, q=24) == RT_ERR_INVALID      # 16-byte rows
    assert _call(native, 1, 1000, 128, f32, 10, big, excl=16, words=31) == RT_ERR_INVALID  # < ceil(1000 / 32)
    assert _call(native, 1, 1000, 128, f32, 10, big, ws=None) == RT_ERR_WORKSPACE
    assert _call(native, 0, 1000, 128, f32, 10, 0, ws=None) == RT_OK               # no queries: nothing to do


@pytest.mark.parametrize("nq,nx,k", [(1, 1000, 50), (8, 10**6, 128), (3, 4097, 100), (1, 0, 10)])
def test_one_byte_less_than_the_size_query_is_refused(native, nq, nx, k):
    for dtype in DTYPES:
        code = native.dtype_code(dtype)
        need = native.lib().rt_flatip_topk_online_workspace_bytes(nq, nx, 128, code, k)
        _, blocks, _ = _plan(native, nq, nx, 128, code, k)
        assert need >= nq * k * blocks * 8  # [nq][k][blocks] composite keys
        assert _call(native, nq, nx, 128, code, k, need - 1) == RT_ERR_WORKSPACE


def test_wrapper_refuses_cpu_tensors(native):
    from rtrec_amd import kernels
    q, x = torch.zeros(1, 128), torch.zeros(100, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.flatip_topk_online(q, x, 10)


def test_limits_are_restated_consistently(native):
    from rtrec_amd import kernels
    from rtrec_amd.serving.retrieval import OnlineSearcher
    assert kernels.ONLINE_MAX_NQ == OnlineSearcher.MAX_BATCH == 8
    assert kernels.ONLINE_MAX_K == OnlineSearcher.MAX_K == 128
    assert _plan(native, kernels.ONLINE_MAX_NQ, 1000, 128, native.RT_F32, kernels.ONLINE_MAX_K)[0] == RT_OK
