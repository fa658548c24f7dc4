"""rt_segment_mean_f32 and rt_ivf_topk (csrc/ivf.hip) on hand-made lists, no
training involved: 16 lists over 3,000 rows whose lengths hold 0, 1, 63, 64,
65, 255, 256, 257 and one list longer than a chunk (the chunk is read from
rt_ivf_topk_plan), stored in a random permutation of the original order.

Every search comparison is np.array_equal on ids AND on scores against
oracle/flatip.c: with every list probed the result is the Flat search over the
original-order corpus; with fewer it is the Flat search restricted to the
probed lists (tests/_ivf_ref.py). The 16-bit scans take the same fmaf chain
over the widened elements, so they are bit-exact too."""
import functools

import numpy as np
import pytest
import torch

import _ivf_ref as ref
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
DT_IDS = ["f32", "f16", "bf16"]
NEG = -np.finfo(np.float32).max
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 100, 30, 200, 150, 90, 300, 469]
NLIST, N = len(LENGTHS), sum(LENGTHS)
EMPTY_LIST, LONG_LIST = 0, 8
CASES = [(dt, d) for dt in DTYPES for d in ((4, 32, 132, 256) if dt == F32 else (8, 32, 136, 256))]
CASE_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-d{d}" for dt, d in CASES]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    assert N == 3000
    chunks, rows_per_chunk, _ = kernels.ivf_topk_plan(1, NLIST, max(LENGTHS))
    assert LENGTHS[LONG_LIST] > rows_per_chunk and chunks > 1, "one list must span several chunks"
    return kernels


def _bits(t):
    """What the oracle takes for a tensor: (array, dtype_code)."""
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


@functools.lru_cache(maxsize=None)
def _layout(seed=0):
    """(offsets [17], row_pos [N] int32, assignment [N] by original position)."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    row_pos = rng.permutation(N).astype(np.int32)
    assignment = np.empty(N, np.int64)
    assignment[row_pos] = np.repeat(np.arange(NLIST), LENGTHS)
    return offsets, row_pos, assignment


@functools.lru_cache(maxsize=None)
def _case(dt, d, equal=False):
    """CPU tensors in ``dt``: queries [33, d], corpus x [N, d] in ORIGINAL order."""
    rng = np.random.default_rng(100 * d + DTYPES.index(dt))
    q = torch.from_numpy(rng.standard_normal((33, d)).astype(np.float32)).to(dt)
    x = rng.standard_normal((N, d)).astype(np.float32)
    if equal:
        x[:] = x[0]
    return q, torch.from_numpy(x).to(dt)


@functools.lru_cache(maxsize=None)
def _flat_oracle(dt, d, equal=False):
    q, x = _case(dt, d, equal)
    qa, code = _bits(q)
    return orc.flat_ip_search(qa, _bits(x)[0], 128, dtype_code=code, nthreads=16)


def _device_lists(x):
    offsets, row_pos, _ = _layout()
    stored = x[torch.from_numpy(row_pos.astype(np.int64))].contiguous()
    return stored.cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(row_pos).cuda()


def _all_probes(nq, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(NLIST) for _ in range(nq)]).astype(np.int64)


def _assert_equal(got, rs, ri, what=""):
    torch.cuda.synchronize()
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), what


# ---- rt_segment_mean_f32 -------------------------------------------------------
@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_segment_mean(K, dt, d):
    """Against numpy fp64 means of the stored (widened) values, within 1 ulp of
    fp32; an empty segment returns prev; normalize gives norm 1 within 1e-6; two
    runs give identical bits."""
    _, x = _case(dt, d)
    offsets = _layout()[0]
    xd, od = x.cuda(), torch.from_numpy(offsets).cuda()
    prev = torch.from_numpy(np.random.default_rng(3).standard_normal((NLIST, d)).astype(np.float32)).cuda()
    x64 = x.double().numpy()
    want = np.stack([x64[offsets[s]:offsets[s + 1]].mean(axis=0) if LENGTHS[s] else prev[s].cpu().double().numpy()
                     for s in range(NLIST)])
    got = K.segment_mean(xd, od, prev)
    again = K.segment_mean(xd, od, prev)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), again.cpu().numpy().view(np.uint32))
    assert np.array_equal(g[EMPTY_LIST], prev[EMPTY_LIST].cpu().numpy())
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(g.astype(np.float64) - want) <= ulp).all(), float((np.abs(g - want) / ulp).max())
    gn = K.segment_mean(xd, od, prev, normalize=True).cpu().numpy()
    nz = np.array(LENGTHS) > 0
    assert np.abs(np.linalg.norm(gn[nz].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    wn = want[nz] / np.linalg.norm(want[nz], axis=1, keepdims=True)
    assert np.abs(gn[nz] - wn).max() <= 2e-7
    assert np.array_equal(gn[EMPTY_LIST], prev[EMPTY_LIST].cpu().numpy())   # prev is copied, not rescaled


# ---- rt_ivf_topk ---------------------------------------------------------------
@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_every_list_probed_is_the_flat_search(K, dt, d):
    """nprobe = nlist, probes in a shuffled order per query: scores (as bits) and
    ids equal flat_ip_search on the original-order corpus. The rows are i.i.d.
    normal (no exact ties), so the oracle's top-128 of 33 queries holds every
    smaller case as a prefix."""
    q, x = _case(dt, d)
    rs, ri = _flat_oracle(dt, d)
    stored, od, pd = _device_lists(x)
    qd = q.cuda()
    probes = torch.from_numpy(_all_probes(33)).cuda()
    for nq in (1, 3, 8, 33):
        for k in (1, 10, 128):
            got = K.ivf_topk(qd[:nq].contiguous(), stored, od, pd, probes[:nq].contiguous(), max(LENGTHS), k)
            _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nq={nq} k={k}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_probed_lists(K, dt):
    """nprobe in {1, 3} equals the probed-lists reference; a query whose probes
    are the empty list and -1 gets all pads; k larger than the probed rows pads."""
    d = 32
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    xa = _bits(x)[0]
    rng = np.random.default_rng(7)
    for nprobe in (1, 3):
        probes = np.stack([rng.choice(NLIST, nprobe, replace=False) for _ in range(33)]).astype(np.int64)
        probes[0, :] = [EMPTY_LIST] + [-1] * (nprobe - 1)          # nothing to scan
        probes[1, :] = [1] + [-1] * (nprobe - 1)                   # the one-row list: k > rows
        probes[2, :] = [LONG_LIST] + [NLIST + 5] * (nprobe - 1)    # out of range: skipped
        for k in (10, 128):
            rs, ri = ref.probed_lists_search(qa, xa, assignment, probes, k, dtype_code=code)
            assert (ri[0] == -1).all() and (rs[0] == NEG).all()
            assert ri[1, 0] >= 0 and (ri[1, 1:] == -1).all()
            got = K.ivf_topk(q.cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), max(LENGTHS), k)
            _assert_equal(got, rs, ri, f"nprobe={nprobe} k={k}")


@pytest.mark.parametrize("tiles", [0, 4], ids=["chunk-default", "chunk-4-tiles"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_all_equal_rows_and_multi_tile_blocks(K, dt, tiles):
    """An all-equal-rows corpus returns ids ascending by ORIGINAL position across
    lists (the tie rule lives in the key, the storage order does not leak). With
    the chunk floor at 4 tiles one block walks the 700-row list in three tiles:
    its candidate buffer fills past its room and is compacted between tiles, on
    massive ties and on random rows."""
    d = 32
    try:
        K.ivf_topk_tuning(tiles)
        chunks, rpc, _ = K.ivf_topk_plan(1, NLIST, max(LENGTHS))
        assert (rpc == 1024 and chunks == 1) if tiles else rpc == 256
        for equal in (True, False):
            q, x = _case(dt, d, equal)
            rs, ri = _flat_oracle(dt, d, equal)
            if equal:
                assert np.array_equal(ri[0], np.arange(128))
            stored, od, pd = _device_lists(x)
            probes = torch.from_numpy(_all_probes(8, seed=2)).cuda()
            for k in (10, 128):
                got = K.ivf_topk(q[:8].cuda(), stored, od, pd, probes, max(LENGTHS), k)
                _assert_equal(got, rs[:8, :k], ri[:8, :k], f"equal={equal} k={k}")
    finally:
        K.ivf_topk_tuning(0)


def test_exclude_bits(K):
    """exclude_bits (indexed by original position) that mask one whole probed
    list, and then everything."""
    dt, d, k = F32, 32, 128
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    nq = 3
    probes = np.array([[LONG_LIST, 5, 2], [7, LONG_LIST, 3], [4, 6, LONG_LIST]], np.int64)
    mask = np.zeros((nq, N), bool)
    mask[:, assignment == LONG_LIST] = True
    mask[1, ::3] = True
    for m in (mask, np.ones((nq, N), bool)):
        bits = ref.bitmap_of_excluded(m)
        rs, ri = ref.probed_lists_search(q[:nq].numpy(), x.numpy(), assignment, probes, k, exclude_bits=bits)
        got = K.ivf_topk(q[:nq].cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), max(LENGTHS), k,
                         exclude_bits=torch.from_numpy(bits.view(np.int32)).cuda())
        _assert_equal(got, rs, ri)
        assert not np.isin(got[1].cpu().numpy(), np.nonzero(assignment == LONG_LIST)[0]).any()
    assert (ri == -1).all()


def test_graph_capture(K):
    """Captured in a torch.cuda.graph and replayed twice: the same bits as the eager call."""
    dt, d, k, nq = F16, 32, 10, 3
    q, x = _case(dt, d)
    rs, ri = _flat_oracle(dt, d)
    stored, od, pd = _device_lists(x)
    qd = q[:nq].cuda()
    probes = torch.from_numpy(_all_probes(nq)).cuda()
    ws = torch.empty(K.native.lib().rt_ivf_topk_workspace_bytes(nq, NLIST, max(LENGTHS), k), dtype=torch.uint8,
                     device="cuda")
    out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"),
           torch.empty((nq, k), dtype=torch.int64, device="cuda"))
    eager = K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k, workspace_buf=ws)
    _assert_equal(eager, rs[:nq, :k], ri[:nq, :k], "eager")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            K.ivf_topk(qd, stored, od, pd, probes, max(LENGTHS), k, out=out, workspace_buf=ws)
    for _ in range(2):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        _assert_equal(out, rs[:nq, :k], ri[:nq, :k], "replay")
