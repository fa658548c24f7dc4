"""rt_mmr_rerank alone, against the fp64 reference of _mmr_ref.

Random data is held to ``check_trace`` — every choice of the kernel, replayed in
fp64, is within the derived fp32 bound of the fp64 maximum — because the gap
between the best and the second-best objective falls to 1e-7 on such inputs and a
correct fp32 kernel may then differ from the fp64 sequence. Dyadic data, where
every value is exact in fp32, is held to the fp64 sequence itself, ties included.
The contract cases are bit for bit."""
import numpy as np
import pytest
import torch

import _mmr_ref as mref

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
NEG = np.float32(-np.finfo(np.float32).max)
LAMS = (0.0, 0.3, 0.5, 1.0)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


def _store(rows64, dtype):
    """(device rows in ``dtype``, their stored values as fp64)."""
    t = torch.from_numpy(np.ascontiguousarray(rows64)).to(dtype)
    return t.cuda().contiguous(), t.double().numpy()


def _candidates(stored64, queries64, n_cand):
    """Per query the top ``n_cand`` stored rows by fp64 score, stable: ([nq, C] f32, [nq, C] i64)."""
    pairs = [mref.sorted_candidates(stored64, q, n_cand) for q in queries64]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _run(K, scores, ids, rows_t, k, lam, **kw):
    lam_t = lam if isinstance(lam, float) else torch.tensor(np.asarray(lam, np.float32)).cuda()
    s, p = K.mmr_rerank(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda(), rows_t, k, lam_t, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), p.cpu().numpy()


def _queries(seed, nq, d):
    rng = np.random.default_rng(1000 + seed)
    q = rng.standard_normal((nq, d))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


# ---- shapes: check_trace on every row ----
@DTYPES
@pytest.mark.parametrize("n_cand", [1, 2, 37, 100, 128])
def test_shapes_trace(K, dtype, n_cand):
    nq = 8
    lam = [LAMS[q % 4] for q in range(nq)]
    for d in (4, 8, 64, 256):
        if d == 4 and dtype != F32:
            continue
        for normalize in (False, True):
            rows64, _ = mref.clustered(7 * d + n_cand, max(4 * n_cand, 8), d, unit=not normalize)
            if normalize:
                rows64 *= np.linspace(0.5, 3.0, len(rows64))[:, None]     # norms that differ
                rows64[3] = 0.0                                           # and a zero row
            rows_t, stored = _store(rows64, dtype)
            scores, ids = _candidates(stored, _queries(d, nq, d), n_cand)
            for k in sorted({1, min(10, n_cand), n_cand}):
                out_s, out_p = _run(K, scores, ids, rows_t, k, lam, normalize=normalize)
                assert out_s.shape == (nq, k) and out_p.shape == (nq, k)
                for q in range(nq):
                    mref.check_trace(scores[q], ids[q], stored, k, lam[q], normalize, out_s[q], out_p[q])
                    if lam[q] == 1.0:   # the identity, bit for bit
                        assert np.array_equal(out_p[q], ids[q, :k])
                        assert np.array_equal(out_s[q].view(np.uint32), scores[q, :k].view(np.uint32))


@pytest.mark.parametrize("dtype,n_cand,d,normalize", [(F16, 100, 64, False), (F32, 37, 8, True)],
                         ids=["f16-100x64", "f32-37x8-cos"])
def test_more_blocks_than_cus(K, dtype, n_cand, d, normalize):
    nq, k = 300, 10
    rows64, _ = mref.clustered(11, 1200, d, unit=not normalize)
    rows_t, stored = _store(rows64, dtype)
    scores, ids = _candidates(stored, _queries(3, nq, d), n_cand)
    lam = [LAMS[q % 4] for q in range(nq)]
    out_s, out_p = _run(K, scores, ids, rows_t, k, lam, normalize=normalize)
    for q in range(nq):
        mref.check_trace(scores[q], ids[q], stored, k, lam[q], normalize, out_s[q], out_p[q])


def test_reorders_and_diversifies(K):
    """A kernel that truncates fails here. The recipe: the 100 rows of a seeded
    clustered corpus are the candidates of the query drawn with it; at lambda <=
    0.7 the fp64 reference always reorders the top-10 and raises its intra-list
    diversity by 0.0277 or more (seeds 0..49, test_mmr_cpu.py) — four orders of
    magnitude above the trace tolerance, so the kernel's list must gain too."""
    nq, n_cand, d, k = 8, 100, 64, 10
    corpora = [mref.clustered(seed, n_cand, d) for seed in range(nq)]
    rows_t, stored = _store(np.concatenate([c[0] for c in corpora]), F32)
    pairs = [mref.sorted_candidates(stored[q * n_cand:(q + 1) * n_cand], corpora[q][1], n_cand) for q in range(nq)]
    scores = np.stack([p[0] for p in pairs])
    ids = np.stack([p[1] + q * n_cand for q, p in enumerate(pairs)])
    for lam in (0.3, 0.5, 0.7):
        out_s, out_p = _run(K, scores, ids, rows_t, k, lam)
        for q in range(nq):
            mref.check_trace(scores[q], ids[q], stored, k, lam, False, out_s[q], out_p[q])
            assert not np.array_equal(out_p[q], ids[q, :k])
            gain = mref.intra_list_diversity(out_p[q], stored) - mref.intra_list_diversity(ids[q, :k], stored)
            assert gain > 0, (lam, q, gain)


# ---- exact cases: the fp64 sequence itself ----
def _dyadic(seed, n, d):
    """Elements are multiples of 1/8 in [-2, 2]: every product, dot product, score and
    objective (lambda a multiple of 1/4) is exact in fp32, in any order of summation."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-16, 17, size=(n, d)) / 8.0
    q = rng.integers(-16, 17, size=d) / 8.0
    return rows, q


@DTYPES
@pytest.mark.parametrize("n_cand,d", [(37, 8), (100, 64), (128, 32)])
def test_exact_sequences(K, dtype, n_cand, d):
    rows64, q = _dyadic(n_cand + d, 3 * n_cand, d)
    rows64[5] = rows64[2]            # duplicated rows at different positions: equal scores, similarity = |row|^2
    rows64[40 % len(rows64)] = rows64[2]
    rows64[9] = -rows64[8]
    rows64[11] = 0.0                 # a zero row: score 0, similarity 0
    rows_t, stored = _store(rows64, dtype)
    assert np.array_equal(stored, rows64)
    scores, ids = mref.sorted_candidates(stored, q, n_cand)
    assert len(np.unique(scores)) < n_cand          # equal scores are in
    lams = [0.0, 0.25, 0.5, 0.75, 1.0]
    nq = len(lams)
    S, I = np.tile(scores, (nq, 1)), np.tile(ids, (nq, 1))
    for k in (n_cand, min(10, n_cand)):
        out_s, out_p = _run(K, S, I, rows_t, k, lams)
        for r, lam in enumerate(lams):
            want_s, want_p, _ = mref.mmr_select(scores, ids, stored, k, lam)
            assert np.array_equal(out_p[r], want_p), (lam, k)
            assert np.array_equal(out_s[r].view(np.uint32), want_s.view(np.uint32)), (lam, k)


# ---- contract cases ----
def _case(dtype=F16, n=600, d=64, n_cand=100, nq=8, seed=5):
    rows64, _ = mref.clustered(seed, n, d)
    rows_t, stored = _store(rows64, dtype)
    scores, ids = _candidates(stored, _queries(seed, nq, d), n_cand)
    return rows_t, stored, scores, ids


def test_absent_candidates_are_skipped_and_the_tail_is_padded(K):
    d, n_rows, n_pos = 32, 50, 60
    rows64, q = mref.clustered(2, n_rows, d)
    # the rows end an allocation, with poison in front of them: slot -1 would read it
    buf = torch.full(((n_rows + 4) * d,), float("nan"), dtype=F32, device="cuda")
    rows_t = buf[4 * d:].view(n_rows, d)
    rows_t.copy_(torch.from_numpy(rows64).to(F32))
    stored = rows_t.cpu().double().numpy()
    poison = 3                                     # a real row no PRESENT candidate may reach through a bad id
    slot = np.arange(80, dtype=np.int32)           # positions 0..79 -> slots; n_pos = 60 of them are valid
    slot[50:] = poison
    slot[7], slot[9], slot[11] = -1, n_rows, 10 ** 6
    ids = np.array([[65, 1 << 40, 7, 9, 11, 20, -1, 21, 22, 79, 23, 24, 25]], dtype=np.int64)
    scores = np.array([[9, 8, 7, 6, 5, 0.9, NEG, 0.8, 0.7, 0.65, 0.6, 0.5, 0.4]], dtype=np.float32)
    by_pos = {p: stored[p] for p in (20, 21, 22, 23, 24, 25)}
    present = [20, 21, 22, 23, 24, 25]
    for k in (3, 13):
        for lam in (0.5, 1.0):
            out_s, out_p = _run(K, scores, ids, rows_t, k, lam, pos_slot=torch.from_numpy(slot).cuda(), n_pos=n_pos)
            mref.check_trace(scores[0], ids[0], by_pos, k, lam, False, out_s[0], out_p[0])
            got = [int(p) for p in out_p[0] if p >= 0]
            assert set(got) <= set(present) and len(got) == min(k, 6)
            if k == 13:
                assert (out_p[0, 6:] == -1).all() and (out_s[0, 6:] == NEG).all()
            if lam == 1.0:
                assert got == present[:len(got)]
    # the identity map: an id at or past n_pos, or past the rows, is absent
    ids2 = np.array([[n_rows, 70, 5, -1, 6, 49]], dtype=np.int64)
    scores2 = np.array([[3, 2, 0.9, NEG, 0.8, 0.7]], dtype=np.float32)
    out_s, out_p = _run(K, scores2, ids2, rows_t, 6, 1.0)
    assert out_p[0].tolist() == [5, 6, 49, -1, -1, -1] and (out_s[0, 3:] == NEG).all()
    out_s, out_p = _run(K, scores2, ids2, rows_t, 6, 1.0, n_pos=49)          # position 49 leaves too
    assert out_p[0].tolist() == [5, 6, -1, -1, -1, -1]
    out_s, out_p = _run(K, scores2[:, :2], ids2[:, :2], rows_t, 2, 0.5)      # nobody is present
    assert out_p[0].tolist() == [-1, -1] and (out_s[0] == NEG).all()
    assert torch.isnan(buf[: 4 * d]).all()


def test_duplicate_positions(K):
    rows_t, stored, scores, ids = _case(n_cand=40, nq=2)
    ids[:, 1], scores[:, 1] = ids[:, 0], scores[:, 0]       # a list probed twice: the same row again
    ids[:, 7], scores[:, 7] = ids[:, 6], scores[:, 6]
    for lam in (0.3, 1.0):
        out_s, out_p = _run(K, scores, ids, rows_t, 40, lam)
        for q in range(2):
            chosen = mref.check_trace(scores[q], ids[q], stored, 40, lam, False, out_s[q], out_p[q])
            assert sorted(chosen) == list(range(40))        # each duplicate is chosen once, as its own candidate
            assert sorted(out_p[q].tolist()) == sorted(ids[q].tolist())


@DTYPES
@pytest.mark.parametrize("normalize", [False, True], ids=["ip", "cos"])
def test_pos_slot_permutation_is_the_identity_case(K, dtype, normalize):
    rows_t, stored, scores, ids = _case(dtype=dtype)
    n = rows_t.shape[0]
    perm = np.random.default_rng(1).permutation(n)            # stored row s holds position perm[s]
    slot = np.empty(n, np.int32)
    slot[perm] = np.arange(n, dtype=np.int32)
    rows_perm = rows_t[torch.from_numpy(perm).cuda()].contiguous()
    lam = [LAMS[q % 4] for q in range(len(ids))]
    a = _run(K, scores, ids, rows_t, 10, lam, normalize=normalize)
    b = _run(K, scores, ids, rows_perm, 10, lam, pos_slot=torch.from_numpy(slot).cuda(), normalize=normalize)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_row_index_batch_size_and_repetition_do_not_matter(K):
    rows_t, _, scores, ids = _case(dtype=BF16, d=128, n_cand=128)
    lam = [0.4] * 8
    full = _run(K, scores, ids, rows_t, 20, lam, normalize=True)
    again = _run(K, scores, ids, rows_t, 20, lam, normalize=True)
    alone = _run(K, scores[5:6].copy(), ids[5:6].copy(), rows_t, 20, 0.4, normalize=True)
    for x, y in ((full, again), ((full[0][5:6], full[1][5:6]), alone)):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))


def test_captured_graph_follows_lambda_changed_in_place(K):
    rows_t, stored, scores, ids = _case(dtype=F32, nq=4)
    s_t, p_t = torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda()
    lam_t = torch.full((4,), 1.0, dtype=F32, device="cuda")
    out = (torch.empty((4, 10), dtype=F32, device="cuda"), torch.empty((4, 10), dtype=torch.int64, device="cuda"))
    K.mmr_rerank(s_t, p_t, rows_t, 10, lam_t, out=out)        # eager first: the kernel is loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.mmr_rerank(s_t, p_t, rows_t, 10, lam_t, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), ids[:, :10])  # lambda = 1: the identity
    lam_t.copy_(torch.tensor([0.3, 0.5, 1.0, 0.0], device="cuda"))
    g.replay()
    torch.cuda.synchronize()
    got_s, got_p = out[0].cpu().numpy(), out[1].cpu().numpy()
    for q, lam in enumerate((0.3, 0.5, 1.0, 0.0)):
        mref.check_trace(scores[q], ids[q], stored, 10, lam, False, got_s[q], got_p[q])
    assert not np.array_equal(got_p[0], ids[0, :10]) and not np.array_equal(got_p[1], ids[1, :10])
    assert np.array_equal(got_p[2], ids[2, :10]) and got_p[3, 0] == ids[3, 0]
    eager = _run(K, scores, ids, rows_t, 10, [0.3, 0.5, 1.0, 0.0])
    assert np.array_equal(eager[1], got_p) and np.array_equal(eager[0].view(np.uint32), got_s.view(np.uint32))


def test_lambda_is_clamped(K):
    rows_t, _, scores, ids = _case(nq=2)
    out = _run(K, scores, ids, rows_t, 10, [7.0, -3.0])
    want = _run(K, scores, ids, rows_t, 10, [1.0, 0.0])
    assert np.array_equal(out[1], want[1])
