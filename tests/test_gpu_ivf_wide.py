"""rt_ivf_topk_wide (csrc/ivf_wide.hip) on hand-made lists, no training: 8 lists
of 0, 1, 37, 255, 256, 257, 600 and 3000 rows stored in a random permutation of
the original order; the 3000-row list is stored in ascending score order for
query 0, so every one of its rows passes the threshold. At the default plan a
chunk is one 256-row tile (every block is selection-free for k >= 256); with the
chunk floor at 16 tiles the 3000-row list is one block whose 2,048-key buffer
compacts more than once. Scores (as bits) and ids equal the C oracle restricted
to the probed rows (_ivf_ref.probed_lists_search) for every k, and
kernels.ivf_topk for k <= 128."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _ivf_ref as ref

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
LENGTHS = [0, 1, 37, 255, 256, 257, 600, 3000]
NLIST, N, ASC_LIST, MLR = len(LENGTHS), sum(LENGTHS), 7, max(LENGTHS)
KS = [1, 128, 129, 256, 1000, 1024]
floors = pytest.mark.parametrize("min_tiles", [0, 16], ids=["chunk1", "chunk16"])


@pytest.fixture()
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels
    yield kernels
    kernels.ivf_topk_tuning(0)


def _oracle_bits(t):
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), (1 if t.dtype == F16 else 2)


@functools.lru_cache(maxsize=None)
def _case(dt, d, dyadic=False):
    """CPU: queries [5, d] and corpus [N, d] (ORIGINAL order) in ``dt``, offsets,
    row_pos (list ASC_LIST ascending in query 0's score), assignment by position."""
    rng = np.random.default_rng(10 * d + [F32, F16, BF16].index(dt) + (5 if dyadic else 0))
    draw = (lambda s: rng.integers(-32, 33, s) / 16.0) if dyadic else rng.standard_normal
    q, x = draw((5, d)).astype(np.float32), draw((N, d)).astype(np.float32)
    if dyadic:   # half the rows are copies of 4 vectors that score highest for query 0, spread over all lists
        four = np.repeat(2.0 * np.sign(q[:1]), 4, axis=0)
        four[np.arange(4), np.arange(4)] = 0.0
        few = rng.random(N) < 0.5
        x[few] = four[rng.integers(0, 4, int(few.sum()))]
    q, x = torch.from_numpy(q).to(dt), torch.from_numpy(x).to(dt)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    row_pos = rng.permutation(N).astype(np.int32)
    lo, hi = offsets[ASC_LIST], offsets[ASC_LIST + 1]
    s0 = x[row_pos[lo:hi].astype(np.int64)].double().numpy() @ q[0].double().numpy()
    row_pos[lo:hi] = row_pos[lo:hi][np.argsort(s0, kind="stable")]
    assignment = np.empty(N, np.int64)
    assignment[row_pos] = np.repeat(np.arange(NLIST), LENGTHS)
    return q, x, offsets, row_pos, assignment


def _probes(nq, nprobe, rng):
    """Query 0 probes the ascending list first and, with nprobe > 1, ends with an entry
    >= nlist; with nq = 5 query 1 probes the lists of 1, 0 and 37 rows first (fewer
    than k rows: pads) and the last query starts with -1."""
    p = np.stack([rng.permutation(NLIST) for _ in range(nq)]).astype(np.int64)
    p[0] = [ASC_LIST] + [l for l in p[0] if l != ASC_LIST]
    if nq > 1:
        p[1] = [1, 0, 2] + [l for l in p[1] if l not in (0, 1, 2)]
        p[nq - 1, 0] = -1
    p = np.ascontiguousarray(p[:, :nprobe])
    if nprobe > 1:
        p[0, nprobe - 1] = NLIST + 2
    return p


def _equal(got, rs, ri, what):
    torch.cuda.synchronize()
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, ri), what
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), what


def _sweep(K, dt, d, min_tiles, dyadic, ks):
    K.ivf_topk_tuning(min_tiles)
    _, rows_per_chunk, _ = K.ivf_topk_plan(1, 8, MLR)
    assert rows_per_chunk == (256 if min_tiles == 0 else 4096)
    q, x, offsets, row_pos, assignment = _case(dt, d, dyadic)
    stored = x[torch.from_numpy(row_pos.astype(np.int64))].contiguous().cuda()
    od, pd = torch.from_numpy(offsets).cuda(), torch.from_numpy(row_pos).cuda()
    (qa, code), xa = _oracle_bits(q), _oracle_bits(x)[0]
    rng = np.random.default_rng(5)
    for nq, nprobe in itertools.product([1, 5], [1, 3, 8]):
        probes = _probes(nq, nprobe, rng)
        prd, qd = torch.from_numpy(probes).cuda(), q[:nq].cuda()
        rs, ri = ref.probed_lists_search(qa[:nq], xa, assignment, probes, max(ks), dtype_code=code)
        if nq > 1 and nprobe == 3:
            assert (ri[1, 38:] == -1).all() and ri[1, 37] >= 0   # lists of 1, 0 and 37 rows: pads
        mask = np.zeros((nq, N), bool)   # each query's best 5
        for i in range(nq):
            mask[i, ri[i, :5][ri[i, :5] >= 0]] = True
        bits = ref.bitmap_of_excluded(mask)
        xs, xi = ref.probed_lists_search(qa[:nq], xa, assignment, probes, max(ks), exclude_bits=bits, dtype_code=code)
        for (want_s, want_i, eb), k in itertools.product(
                [(rs, ri, None), (xs, xi, torch.from_numpy(bits.view(np.int32)).cuda())], ks):
            what = f"nq={nq} nprobe={nprobe} k={k} excl={eb is not None}"
            got = K.ivf_topk_wide(qd, stored, od, pd, prd, MLR, k, exclude_bits=eb)
            _equal(got, want_s[:, :k], want_i[:, :k], what)
            if k <= K.IVF_MAX_K:
                old = K.ivf_topk(qd, stored, od, pd, prd, MLR, k, exclude_bits=eb)
                assert torch.equal(got[0], old[0]) and torch.equal(got[1], old[1]), what


@floors
@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_wide_search(K, dt, d, min_tiles):
    _sweep(K, dt, d, min_tiles, False, KS)


@floors
def test_tie_groups_split_by_position(K, min_tiles):
    """Multiples of 2^-4 (every fp32 sum exact), half the rows copies of 4 vectors
    spread over all lists: the k-th boundary falls inside a tie group that spans
    many blocks, and ids come position-ascending within it, as the oracle's."""
    q, x, _, _, assignment = _case(F32, 32, True)
    rs, _ = ref.probed_lists_search(q[:1].numpy(), x.numpy(), assignment, np.array([[ASC_LIST]]), 1001)
    assert all(rs[0, k - 1] == rs[0, k] for k in (129, 300, 1000))   # every boundary inside a tie group
    _sweep(K, F32, 32, min_tiles, True, [129, 300, 1000])


def test_lists_with_slack(K):
    """list_len / n_pos: every list has 7 slots of slack that hold high-scoring rows
    with VALID positions (only list_len keeps them out), and the 10 highest
    positions are stale (>= n_pos): dropped."""
    q, x, offsets, row_pos, assignment = _case(F32, 32)
    n_pos, slack = N - 10, 7
    cap_off = offsets + slack * np.arange(NLIST + 1)
    cap = int(cap_off[-1])
    stored = torch.full((cap, 32), 4.0)
    rp = np.random.default_rng(3).integers(0, n_pos, cap).astype(np.int32)
    for l in range(NLIST):
        a, b = int(offsets[l]), int(offsets[l + 1])
        stored[cap_off[l]:cap_off[l] + b - a] = x[torch.from_numpy(row_pos[a:b].astype(np.int64))]
        rp[cap_off[l]:cap_off[l] + b - a] = row_pos[a:b]
    probes = _probes(5, 8, np.random.default_rng(9))
    args = (q.cuda(), stored.cuda(), torch.from_numpy(cap_off).cuda(), torch.from_numpy(rp).cuda(),
            torch.from_numpy(probes).cuda(), MLR + slack)
    lens = dict(list_len=torch.tensor(LENGTHS, dtype=torch.int64).cuda(), n_pos=n_pos)
    for k in (129, 1024):
        rs, ri = ref.probed_lists_search(q.numpy(), x.numpy()[:n_pos], assignment[:n_pos], probes, k)
        _equal(K.ivf_topk_wide(*args, k, **lens), rs, ri, f"k={k}")


def test_graph_capture(K):
    """Captured in a torch.cuda.graph and replayed three times: the eager result."""
    nq, k, nprobe = 5, 300, 8
    q, x, offsets, row_pos, _ = _case(F16, 32)
    probes = _probes(nq, nprobe, np.random.default_rng(2))
    ops = (q.cuda(), x[torch.from_numpy(row_pos.astype(np.int64))].contiguous().cuda(), torch.from_numpy(offsets).cuda(),
           torch.from_numpy(row_pos).cuda(), torch.from_numpy(probes).cuda(), MLR, k)
    ws = torch.empty(K.native.lib().rt_ivf_topk_wide_workspace_bytes(nq, nprobe, MLR, k), dtype=torch.uint8,
                     device="cuda")
    eager = K.ivf_topk_wide(*ops, workspace_buf=ws)
    torch.cuda.synchronize()
    es, ei = eager[0].clone(), eager[1].clone()
    out = (torch.empty_like(es), torch.empty_like(ei))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            K.ivf_topk_wide(*ops, out=out, workspace_buf=ws)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], es) and torch.equal(out[1], ei)
