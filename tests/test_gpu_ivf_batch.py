"""rt_ivf_topk_batch (csrc/ivf_batch.hip), the list-major batch search, on
hand-made lists with no training: 16 lists over 3,000 rows whose lengths hold
0, 1, 63, 64, 65, 255, 256, 257 and one list longer than a chunk (the chunk is
read from rt_ivf_topk_batch_plan), stored in a random permutation of the
original order.

Every comparison is np.array_equal on ids AND on the uint32 view of the scores,
over every query, against oracle/flatip.c: with every list probed the result is
the Flat search over the original-order corpus; with fewer it is the Flat
search restricted to the probed lists (tests/_ivf_ref.py). kernels.ivf_topk, the
per-query scan, is a second witness on the same operands. Every call runs with
guard bands of a sentinel pattern behind out_scores, out_ids and the workspace,
which must be intact afterwards."""
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
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1100, 100, 30, 200, 150, 90, 300, 69]
NLIST, N = len(LENGTHS), sum(LENGTHS)
EMPTY_LIST, ONE_ROW_LIST, LONG_LIST = 0, 1, 8
MLR = max(LENGTHS)
NQ = 65   # 2 QT + 1
CASES = [(dt, d) for dt in DTYPES for d in ((4, 32, 132, 256) if dt == F32 else (8, 32, 136, 256))]
CASE_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-d{d}" for dt, d in CASES]
GUARD = 1024  # bytes


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    assert N == 3000
    qt, rows_per_chunk, chunks, _, _ = kernels.ivf_topk_batch_plan(NQ, NLIST, NLIST, MLR, 128)
    assert qt == 32 and NQ == 2 * qt + 1
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
def _case(dt, d, equal=False, nq=NQ):
    """CPU tensors in ``dt``: queries [nq, d], corpus x [N, d] in ORIGINAL order;
    ``equal``: every row of the long list is the same row."""
    rng = np.random.default_rng(100 * d + DTYPES.index(dt))
    q = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).to(dt)
    x = rng.standard_normal((N, d)).astype(np.float32)
    if equal:
        x[_layout()[2] == LONG_LIST] = x[0]
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


def _guarded(nbytes, dtype):
    """(view of the first nbytes as ``dtype``, the whole uint8 buffer): 0xA5 everywhere."""
    raw = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return raw[:nbytes].view(dtype), raw


def _batch(K, q, stored, od, pd, probes, k, mlr=MLR, **kw):
    """kernels.ivf_topk_batch into guarded outputs and a guarded workspace of exactly
    the size the library asks for; the guard bands are checked after the call."""
    nq, nprobe = probes.shape
    nlist = od.numel() - 1
    W = K.native.lib().rt_ivf_topk_batch_workspace_bytes(nq, nprobe, nlist, mlr, k)
    s, s_raw = _guarded(nq * k * 4, torch.float32)
    i, i_raw = _guarded(nq * k * 8, torch.int64)
    ws, ws_raw = _guarded(W, torch.uint8)
    out = (s.view(nq, k), i.view(nq, k))
    got = K.ivf_topk_batch(q, stored, od, pd, probes, mlr, k, out=out, workspace_buf=ws, **kw)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    for raw, n in ((s_raw, nq * k * 4), (i_raw, nq * k * 8), (ws_raw, W)):
        assert bool((raw[n:] == 0xA5).all()), "guard band overwritten"
    return got


# ---- every list probed: the Flat search -----------------------------------------
@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_every_list_probed_is_the_flat_search(K, dt, d):
    """nprobe = nlist = 16, probes in a shuffled order per query: scores (as bits)
    and ids equal flat_ip_search on the original-order corpus, for nq in {1, QT -
    1, QT, QT + 1, 2 QT + 1} and k in {1, 10, 100, 128}. The rows are i.i.d.
    normal (no exact ties), so the oracle's top-128 of 65 queries holds every
    smaller case as a prefix."""
    q, x = _case(dt, d)
    rs, ri = _flat_oracle(dt, d)
    stored, od, pd = _device_lists(x)
    qd = q.cuda()
    probes = torch.from_numpy(_all_probes(NQ)).cuda()
    for nq in (1, 31, 32, 33, 65):
        for k in (1, 10, 100, 128):
            got = _batch(K, qd[:nq].contiguous(), stored, od, pd, probes[:nq].contiguous(), k)
            _assert_equal(got, rs[:nq, :k], ri[:nq, :k], f"nq={nq} k={k}")


# ---- fewer probes -------------------------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_probed_lists(K, dt, nprobe):
    """nprobe in {1, 3} equals the probed-lists reference and the per-query scan;
    probe rows with -1, nlist and negative garbage entries are skipped; a query
    whose probes name nothing gets all pads; k larger than the probed rows pads."""
    d = 32
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    xa = _bits(x)[0]
    rng = np.random.default_rng(7)
    probes = np.stack([rng.choice(NLIST, nprobe, replace=False) for _ in range(NQ)]).astype(np.int64)
    probes[0, :] = [EMPTY_LIST] + [-1] * (nprobe - 1)             # nothing to scan
    probes[1, :] = [ONE_ROW_LIST] + [-1] * (nprobe - 1)           # the one-row list: k > rows
    probes[2, :] = [LONG_LIST] + [NLIST] * (nprobe - 1)           # nlist itself: out of range
    probes[3, :] = [-7] * (nprobe - 1) + [5]                      # negative garbage first
    probes[4, :] = [-2**40] * (nprobe - 1) + [2**40]              # nothing valid at all
    probes[40, :] = -1
    pdv = torch.from_numpy(probes).cuda()
    for k in (10, 128):
        rs, ri = ref.probed_lists_search(qa, xa, assignment, probes, k, dtype_code=code)
        assert (ri[0] == -1).all() and (rs[0] == NEG).all() and (ri[4] == -1).all() and (ri[40] == -1).all()
        assert ri[1, 0] >= 0 and (ri[1, 1:] == -1).all()
        got = _batch(K, q.cuda(), stored, od, pd, pdv, k)
        _assert_equal(got, rs, ri, f"nprobe={nprobe} k={k}")
        witness = K.ivf_topk(q.cuda(), stored, od, pd, pdv, MLR, k)
        _assert_equal(got, witness[0].cpu().numpy(), witness[1].cpu().numpy(), f"witness nprobe={nprobe} k={k}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_one_list_for_all_queries_and_one_list_each(K, dt):
    """300 queries that all probe the same single list (ten query tiles over one
    list, two chunks each, while 15 lists go unprobed), and 16 queries that each
    name a different list (16 work items of one query)."""
    d, k = 32, 100
    q, x = _case(dt, d, nq=300)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    xa = _bits(x)[0]
    probes = np.full((300, 1), LONG_LIST, np.int64)
    rs, ri = ref.probed_lists_search(qa, xa, assignment, probes, k, dtype_code=code)
    assert np.isin(ri, np.nonzero(assignment == LONG_LIST)[0]).all()
    got = _batch(K, q.cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), k)
    _assert_equal(got, rs, ri, "one list")
    probes = np.random.default_rng(3).permutation(NLIST).astype(np.int64).reshape(NLIST, 1)
    rs, ri = ref.probed_lists_search(qa[:NLIST], xa, assignment, probes, k, dtype_code=code)
    got = _batch(K, q[:NLIST].cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), k)
    _assert_equal(got, rs, ri, "one list each")
    pads = (ri == -1).sum(axis=1)
    assert pads.max() == k and pads.min() == 0   # the empty list and lists above k rows are both among them


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_all_equal_rows_in_the_long_list(K, dt):
    """Every row of the 1,100-row list is the same row: a massive tie that spans
    both chunks of the list and all three query tiles, resolved by ORIGINAL
    position (the storage order does not leak), with every list probed and with
    the long list alone."""
    d = 32
    q, x = _case(dt, d, equal=True)
    rs, ri = _flat_oracle(dt, d, equal=True)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    probes = torch.from_numpy(_all_probes(NQ, seed=2)).cuda()
    for k in (10, 128):
        got = _batch(K, q.cuda(), stored, od, pd, probes, k)
        _assert_equal(got, rs[:, :k], ri[:, :k], f"all lists k={k}")
    qa, code = _bits(q)
    only = np.full((NQ, 1), LONG_LIST, np.int64)
    rs1, ri1 = ref.probed_lists_search(qa, _bits(x)[0], assignment, only, 128, dtype_code=code)
    assert np.array_equal(ri1[0], np.sort(np.nonzero(assignment == LONG_LIST)[0])[:128])
    got = _batch(K, q.cuda(), stored, od, pd, torch.from_numpy(only).cuda(), 128)
    _assert_equal(got, rs1, ri1, "the long list alone")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_exclude_bits(K, dt):
    """exclude_bits (indexed by original position): one whole probed list masked,
    a stride of positions masked for one query, one query that excludes every
    row it probes, and then everything for everyone."""
    d, k = 32, 128
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    rng = np.random.default_rng(11)
    others = np.setdiff1d(np.arange(NLIST), [LONG_LIST])   # no list twice in a probe row
    probes = np.stack([np.concatenate([[LONG_LIST], rng.choice(others, 2, replace=False)])
                       for _ in range(NQ)]).astype(np.int64)
    mask = np.zeros((NQ, N), bool)
    mask[::2, assignment == LONG_LIST] = True
    mask[1, ::3] = True
    mask[5, np.isin(assignment, probes[5])] = True   # every probed row of query 5
    for m in (mask, np.ones((NQ, N), bool)):
        bits = ref.bitmap_of_excluded(m)
        rs, ri = ref.probed_lists_search(qa, _bits(x)[0], assignment, probes, k, exclude_bits=bits, dtype_code=code)
        got = _batch(K, q.cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), k,
                     exclude_bits=torch.from_numpy(bits.view(np.int32)).cuda())
        _assert_equal(got, rs, ri)
        assert (ri[5] == -1).all()
        assert not np.isin(got[1].cpu().numpy()[::2], np.nonzero(assignment == LONG_LIST)[0]).any()
    assert (ri == -1).all()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_lists_with_slack(K, dt):
    """list_len / n_pos over lists stored with slack: every list owns len + 40
    slots (the empty list too), the slots behind the live rows hold row_pos = -1
    and rows of NaN. The result equals that of the compacted lists (and the
    oracle's), with and without a bitmap; max_list_rows bounds the capacity."""
    d, k = 32, 128
    q, x = _case(dt, d)
    offsets, row_pos, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    slack = 40
    caps = np.array(LENGTHS) + slack
    s_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    total = int(s_off[-1])
    s_rows = torch.full((total, d), float("nan"), dtype=dt)
    s_pos = np.full(total, -1, np.int32)
    for l in range(NLIST):
        a, b = offsets[l], offsets[l + 1]
        s_rows[s_off[l]:s_off[l] + (b - a)] = stored[a:b].cpu()
        s_pos[s_off[l]:s_off[l] + (b - a)] = row_pos[a:b]
    lens = torch.tensor(LENGTHS, dtype=torch.int64).cuda()
    rng = np.random.default_rng(5)
    probes = np.stack([rng.choice(NLIST, 3, replace=False) for _ in range(NQ)]).astype(np.int64)
    probes[0] = [EMPTY_LIST, LONG_LIST, ONE_ROW_LIST]
    pdv = torch.from_numpy(probes).cuda()
    mask = np.zeros((NQ, N), bool)
    mask[:, ::5] = True
    for m in (None, mask):
        bits = None if m is None else ref.bitmap_of_excluded(m)
        bd = None if m is None else torch.from_numpy(bits.view(np.int32)).cuda()
        rs, ri = ref.probed_lists_search(qa, _bits(x)[0], assignment, probes, k, exclude_bits=bits, dtype_code=code)
        compact = _batch(K, q.cuda(), stored, od, pd, pdv, k, exclude_bits=bd)
        _assert_equal(compact, rs, ri, "compacted lists")
        got = _batch(K, q.cuda(), s_rows.cuda(), torch.from_numpy(s_off).cuda(), torch.from_numpy(s_pos).cuda(), pdv,
                     k, mlr=int(caps.max()), exclude_bits=bd, list_len=lens, n_pos=N)
        _assert_equal(got, rs, ri, "lists with slack")
        witness = K.ivf_topk(q.cuda(), s_rows.cuda(), torch.from_numpy(s_off).cuda(), torch.from_numpy(s_pos).cuda(),
                             pdv, int(caps.max()), k, exclude_bits=bd, list_len=lens, n_pos=N)
        _assert_equal(got, witness[0].cpu().numpy(), witness[1].cpu().numpy(), "witness")


def test_a_list_named_twice(K):
    """A probe row naming one list twice may repeat its rows, nothing worse: only
    rows of the probed lists, valid positions, descending scores that are the
    rows' own scores; the other queries of the batch are exact."""
    dt, d, k = F32, 32, 128
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    rng = np.random.default_rng(13)
    probes = np.stack([rng.choice(NLIST, 3, replace=False) for _ in range(NQ)]).astype(np.int64)
    probes[7] = [5, 5, 9]
    probes[8] = [LONG_LIST, LONG_LIST, LONG_LIST]
    got = _batch(K, q.cuda(), stored, od, pd, torch.from_numpy(probes).cuda(), k)
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    rs, ri = ref.probed_lists_search(q.numpy(), x.numpy(), assignment, probes, k)
    for qi in (7, 8):
        ids = gi[qi][gi[qi] >= 0]
        assert ids.size and (ids < N).all() and np.isin(assignment[ids], probes[qi]).all()
        assert (np.diff(gs[qi]) <= 0).all()
        # a returned row that the exact search over the probed lists returns too carries its score
        score_of = dict(zip(ri[qi].tolist(), rs[qi].view(np.uint32).tolist()))
        for i, s in zip(ids.tolist(), gs[qi][:ids.size].view(np.uint32).tolist()):
            assert score_of.get(i, s) == s
    rest = np.setdiff1d(np.arange(NQ), [7, 8])
    _assert_equal((got[0][rest], got[1][rest]), rs[rest], ri[rest], "the other queries")


def test_python_layer_refuses_exclude_lists_and_chunks_by_budget(K, monkeypatch):
    """exclude_lists raises and names ivf_topk; with a small workspace budget the
    queries run in chunks and the result does not change."""
    dt, d, k = F16, 32, 10
    q, x = _case(dt, d)
    rs, ri = _flat_oracle(dt, d)
    stored, od, pd = _device_lists(x)
    probes = torch.from_numpy(_all_probes(NQ)).cuda()
    with pytest.raises(ValueError, match="ivf_topk"):
        K.ivf_topk_batch(q.cuda(), stored, od, pd, probes, MLR, k,
                         exclude_lists=(torch.zeros(NQ + 1, dtype=torch.int64).cuda(),
                                        torch.zeros(0, dtype=torch.int32).cuda()))
    whole = K.native.lib().rt_ivf_topk_batch_workspace_bytes(NQ, NLIST, NLIST, MLR, k)
    monkeypatch.setattr(K, "IVF_BATCH_WORKSPACE_BUDGET", whole // 2)
    got = K.ivf_topk_batch(q.cuda(), stored, od, pd, probes, MLR, k)
    _assert_equal(got, rs[:, :k], ri[:, :k], "chunked by the budget")


def test_graph_capture_and_replay_after_in_place_changes(K):
    """Captured in a torch.cuda.graph: a replay equals the eager result; after
    probes and queries are overwritten in place, the next replay equals the
    eager result for the new inputs (the grid depends on host arguments only)."""
    dt, d, k, nq = F16, 32, 10, 40
    q, x = _case(dt, d)
    _, _, assignment = _layout()
    stored, od, pd = _device_lists(x)
    qa, code = _bits(q)
    rng = np.random.default_rng(17)
    probes_a = np.stack([rng.choice(NLIST, 3, replace=False) for _ in range(nq)]).astype(np.int64)
    probes_b = np.full((nq, 3), -1, np.int64)
    probes_b[:, 0] = LONG_LIST                      # another grouping altogether: one list, two tiles
    probes_b[::3, 1] = 5
    want_a = ref.probed_lists_search(qa[:nq], _bits(x)[0], assignment, probes_a, k, dtype_code=code)
    want_b = ref.probed_lists_search(qa[25:25 + nq], _bits(x)[0], assignment, probes_b, k, dtype_code=code)
    qd = q[:nq].cuda().contiguous()
    pdv = torch.from_numpy(probes_a).cuda()
    ws = torch.empty(K.native.lib().rt_ivf_topk_batch_workspace_bytes(nq, 3, NLIST, MLR, k), dtype=torch.uint8,
                     device="cuda")
    out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"),
           torch.empty((nq, k), dtype=torch.int64, device="cuda"))
    eager = K.ivf_topk_batch(qd, stored, od, pd, pdv, MLR, k, workspace_buf=ws)
    _assert_equal(eager, *want_a, "eager")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            K.ivf_topk_batch(qd, stored, od, pd, pdv, MLR, k, out=out, workspace_buf=ws)
    out[0].zero_()
    out[1].zero_()
    g.replay()
    _assert_equal(out, *want_a, "first replay")
    qd.copy_(q[25:25 + nq].cuda())
    pdv.copy_(torch.from_numpy(probes_b).cuda())
    out[0].zero_()
    out[1].zero_()
    g.replay()
    _assert_equal(out, *want_b, "replay after probes and queries changed in place")
    eager_b = K.ivf_topk_batch(qd, stored, od, pd, pdv, MLR, k)
    _assert_equal(eager_b, *want_b, "eager on the new inputs")
