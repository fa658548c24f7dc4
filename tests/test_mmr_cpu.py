"""Host side of the MMR re-rank (rt_mmr_rerank): self-checks of the tests' fp64
reference on hand-written cases, every status code the entry point returns
before any device work (the pointers below are fakes, never dereferenced), the
refusal of CPU tensors, and the ValueErrors of the Python layers. No GPU."""
import numpy as np
import pytest
import torch

import _mmr_ref as mref

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, -1, -2
FLT_MAX = np.float32(np.finfo(np.float32).max)
# fake operands, far enough apart that no two ranges of a small call overlap
P_S, P_I, P_ROWS, P_SLOT, P_LAM, P_OS, P_OI = (j << 24 for j in range(1, 8))


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    nat.lib()
    return nat


def _call(nat, cand_scores=P_S, cand_ids=P_I, nq=2, n_cand=100, rows=P_ROWS, n_rows=1000, d=64, dtype=0,
          pos_slot=None, n_pos=1000, lam=P_LAM, normalize=0, k=10, out_scores=P_OS, out_ids=P_OI):
    return nat.lib().rt_mmr_rerank(cand_scores, cand_ids, nq, n_cand, rows, n_rows, d, dtype, pos_slot, n_pos, lam,
                                   normalize, k, out_scores, out_ids, None)


# ---- the reference, hand-written ----
def _line(n=6, d=4):
    """Rows on a line of growing angle to e0: the similarity falls with the distance in the list."""
    ang = np.linspace(0.0, 1.2, n)
    rows = np.zeros((n, d))
    rows[:, 0], rows[:, 1] = np.cos(ang), np.sin(ang)
    return rows


def test_reference_lambda_one_is_the_identity():
    rows = _line()
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32)
    ids = np.array([3, 1, 5, 0, 2, 4])
    s, i, chosen = mref.mmr_select(scores, ids, rows, 4, 1.0)
    assert chosen == [0, 1, 2, 3] and i.tolist() == [3, 1, 5, 0] and s.tolist() == scores[:4].tolist()
    assert mref.check_trace(scores, ids, rows, 4, 1.0, False, s, i) == chosen


def test_reference_lambda_zero_starts_at_candidate_zero_and_spreads():
    rows = _line()
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32)
    ids = np.arange(6)
    _, i, chosen = mref.mmr_select(scores, ids, rows, 3, 0.0)
    # all objectives are 0 at the first step: the lowest index; then the row farthest from
    # row 0 (the end of the line), then the one farthest from both
    assert chosen[0] == 0 and chosen[1] == 5 and i[0] == 0
    assert chosen[2] in (2, 3)


def test_reference_ties_go_to_the_lowest_candidate_index():
    rows = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    scores = np.array([1.0, 0.5, 0.5, 0.5], np.float32)
    ids = np.array([7, 9, 8, 2])     # position 9 stands before position 8: the INDEX decides, not the id
    rows_by_pos = {7: rows[0], 9: rows[1], 8: rows[2], 2: rows[3]}
    _, i, chosen = mref.mmr_select(scores, ids, rows_by_pos, 4, 0.5)
    assert chosen == [0, 1, 3, 2] and i.tolist() == [7, 9, 2, 8]   # after 9, its duplicate 8 is the worst
    # m_i is 0 only while NOTHING is chosen: afterwards a negative similarity counts as it is
    rows2 = {0: [1.0, 0], 1: [-1.0, 0], 2: [0, 1.0]}
    _, i2, _ = mref.mmr_select(np.array([1, 0.5, 0.5], np.float32), np.array([0, 1, 2]), rows2, 2, 0.5)
    assert i2.tolist() == [0, 1]    # obj(1) = .25 + .5, obj(2) = .25 - 0


def test_reference_pads_and_absent_candidates():
    rows = np.eye(4)
    rows[2] = np.nan                                  # position 2 holds no row
    scores = np.array([0.9, 0.8, -FLT_MAX, 0.7, 0.6], np.float32)
    ids = np.array([1, 2, -1, 9, 3])                  # no row, pad in the middle, outside the positions
    s, i, chosen = mref.mmr_select(scores, ids, rows, 4, 0.7)
    assert chosen == [0, 4] and i.tolist() == [1, 3, -1, -1]
    assert s[:2].tolist() == [np.float32(0.9), np.float32(0.6)] and (s[2:] == -FLT_MAX).all()
    mref.check_trace(scores, ids, rows, 4, 0.7, False, s, i)
    for bad_ids in ([1, 2, -1, -1], [1, 9, -1, -1], [1, 1, -1, -1], [3, 1, -1, -1][::-1]):
        bad_s = np.array([0.9, 0.8, -FLT_MAX, -FLT_MAX], np.float32)
        with pytest.raises(AssertionError):
            mref.check_trace(scores, ids, rows, 4, 0.7, False, bad_s, np.array(bad_ids))
    with pytest.raises(AssertionError):               # the tail must be pads
        mref.check_trace(scores, ids, rows, 4, 0.7, False, np.array([0.9, 0.6, 0.6, -FLT_MAX], np.float32),
                         np.array([1, 3, 3, -1]))


def test_reference_duplicates_and_normalize():
    rows = {4: [2.0, 0.0], 5: [0.0, 3.0], 6: [0.0, 0.0]}
    scores = np.array([1.0, 1.0, 0.9, 0.8], np.float32)
    ids = np.array([4, 4, 5, 6])                      # position 4 twice: two candidates
    _, i, chosen = mref.mmr_select(scores, ids, rows, 4, 0.5, normalize=True)
    # after 4: its duplicate has cosine 1, row 5 cosine 0, the zero row similarity 0 to everything
    assert chosen == [0, 2, 3, 1] and i.tolist() == [4, 5, 6, 4]
    _, i_raw, _ = mref.mmr_select(scores, ids, rows, 2, 0.5, normalize=False)
    assert i_raw.tolist() == [4, 5]                   # raw inner products: 4 . 4 = 4
    got = mref.check_trace(scores, ids, rows, 4, 0.5, True, scores[[0, 2, 3, 1]], i)
    assert sorted(got) == [0, 1, 2, 3]
    assert mref.tolerance(scores, ids, rows) == 2 * (2 + 8) * 2.0 ** -24 * 9.0
    assert abs(mref.tolerance(np.ones(3, np.float32), np.arange(3), np.eye(256)[:3]) - 3.147e-5) < 1e-7


def test_reference_recipe_reorders_and_diversifies():
    """What the GPU tests' data rest on: the 100 rows of a clustered corpus (d = 64)
    as the candidates of the query drawn with it, k = 10. At every lambda <= 0.7 the
    top-10 is reordered and intra-list diversity rises; the smallest gain over seeds
    0..49 is 0.02779 (checked here on the first 12)."""
    for seed in range(12):
        rows, q = mref.clustered(seed, 100, 64)
        s, ids = mref.sorted_candidates(rows, q, 100)
        plain = mref.intra_list_diversity(ids[:10], rows)
        for lam in (0.3, 0.5, 0.7):
            _, out, _ = mref.mmr_select(s, ids, rows, 10, lam)
            assert out.tolist() != ids[:10].tolist()
            assert mref.intra_list_diversity(out, rows) - plain >= 0.0277, (seed, lam)


# ---- the C ABI: every refusal, before any device work ----
def test_symbol_and_signature(native):
    assert hasattr(native.lib(), "rt_mmr_rerank") and len(native.SIGNATURES["rt_mmr_rerank"][1]) == 16
    from rtrec_amd import kernels
    assert kernels.MMR_MAX_CAND == 128 == kernels.ONLINE_MAX_K == kernels.IVF_MAX_K


def test_invalid_arguments(native):
    for bad in ({"cand_scores": None}, {"cand_ids": None}, {"lam": None}, {"out_scores": None}, {"out_ids": None},
                {"rows": None},                                   # rows exist
                {"k": 0}, {"k": -1}, {"n_cand": 0}, {"n_cand": -3}, {"nq": -1}, {"n_rows": -1}, {"n_pos": -1},
                {"d": 0}, {"dtype": 3}, {"dtype": -1},
                {"rows": P_ROWS + 8},                             # 16-byte alignment of the rows
                {"out_scores": P_S}, {"out_ids": P_I},            # aliasing the inputs
                {"out_scores": P_S + 2 * 100 * 4 - 4},            # the last input word
                {"out_ids": P_I + 8}, {"out_scores": P_I}, {"out_ids": P_S}):
        assert _call(native, **bad) == RT_ERR_INVALID, bad
    # refused with no query too: the arguments are checked first
    assert _call(native, nq=0, k=0) == RT_ERR_INVALID
    assert _call(native, nq=0, dtype=9) == RT_ERR_INVALID


def test_unsupported_arguments(native):
    for bad in ({"n_cand": 129, "k": 10}, {"k": 101}, {"n_cand": 5, "k": 6},
                {"d": 260}, {"d": 66}, {"d": 68, "dtype": 1}, {"d": 4, "dtype": 2}, {"d": 257},
                {"n_pos": (1 << 31) - 1}, {"n_pos": 1 << 40}):
        assert _call(native, **bad) == RT_ERR_UNSUPPORTED, bad


def test_accepted_without_device_work(native):
    """nq == 0 is RT_OK whatever else is well-formed: NULL rows with no rows, NULL or
    given pos_slot, every dtype at its d limits."""
    assert _call(native, nq=0) == RT_OK
    assert _call(native, nq=0, rows=None, n_rows=0) == RT_OK
    assert _call(native, nq=0, pos_slot=P_SLOT) == RT_OK
    assert _call(native, nq=0, n_cand=128, k=128, d=256) == RT_OK
    assert _call(native, nq=0, d=4) == RT_OK and _call(native, nq=0, d=8, dtype=1) == RT_OK
    assert _call(native, nq=0, d=256, dtype=2, n_pos=(1 << 31) - 2) == RT_OK
    assert _call(native, nq=0, out_scores=P_S) == RT_OK    # empty ranges do not overlap


# ---- the Python layers ----
def test_wrapper_refuses_cpu_tensors(native):
    from rtrec_amd import kernels
    s, p, rows = torch.zeros(2, 20), torch.zeros(2, 20, dtype=torch.int64), torch.zeros(50, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.mmr_rerank(s, p, rows, 5, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.mmr_rerank(s, p, rows, 5, torch.zeros(2), pos_slot=torch.zeros(50, dtype=torch.int32))


def _index(cls_name="HipFlatIPIndex", **cfg):
    from rtrec_amd.serving import retrieval as R
    return getattr(R, cls_name)({"dimension": 32, **cfg})


@pytest.mark.parametrize("cls_name", ["HipFlatIPIndex", "HipIVFFlatIndex", "HipMutableIVFFlatIndex"])
def test_search_value_errors(cls_name):
    """Checked before anything else, an index that was never built included."""
    index = _index(cls_name)
    q = np.zeros((1, 32), np.float32)
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="0 <= mmr_lambda <= 1"):
            index.search(q, 10, mmr_lambda=lam)
    with pytest.raises(ValueError, match="k <= mmr_candidates <= 128"):
        index.search(q, 10, mmr_lambda=0.5, mmr_candidates=9)          # k > mmr_candidates
    with pytest.raises(ValueError, match="k <= mmr_candidates <= 128"):
        index.search(q, 10, mmr_lambda=0.5, mmr_candidates=129)
    with pytest.raises(ValueError, match="k <= mmr_candidates <= 128"):
        index.search(q, 129, mmr_lambda=0.5)                           # no default can hold k
    with pytest.raises(ValueError, match="filter_ids together with mmr_lambda"):
        index.search(q, 10, filter_ids=["a"], mmr_lambda=0.5)
    with pytest.raises(ValueError, match="without mmr_lambda"):
        index.search(q, 10, mmr_candidates=50)
    with pytest.raises(ValueError, match="not built"):                 # well-formed: the next check is the old one
        index.search(q, 10, mmr_lambda=0.5, mmr_candidates=100)


def test_default_candidates():
    index = _index()
    assert index._mmr_args(10, None, None) is None
    index.current_size = 5000
    assert index._mmr_args(10, 0.5, None) == 100 and index._mmr_args(20, 0.0, None) == 128
    assert index._mmr_args(128, 1.0, None) == 128 and index._mmr_args(10, 0.5, 10) == 10
    index.current_size = 40
    assert index._mmr_args(10, 0.5, None) == 40 and index._mmr_args(50, 0.5, None) == 50


def test_l2_and_sharded_refuse():
    q = np.zeros((1, 32), np.float32)
    with pytest.raises(ValueError, match="L2"):
        _index(metric="l2").search(q, 10, mmr_lambda=0.5)
    sharded = _index("HipShardedFlatIPIndex")
    with pytest.raises(ValueError, match="single-GPU"):
        sharded.search(q, 5, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="single-GPU"):
        sharded._mmr_args(5, 0.5, None)


def test_engine_passes_the_keywords_and_skips_the_cache():
    from rtrec_amd.serving import retrieval as R
    engine = R.RetrievalEngine({"index_type": "hip_flat", "embedding_dim": 32})
    q = np.zeros((1, 32), np.float32)
    with pytest.raises(ValueError, match="0 <= mmr_lambda <= 1"):
        engine.retrieve(q, 10, mmr_lambda=2.0)
    seen = {}

    class Probe:
        current_size = 0

        def search(self, queries, k, filter_ids=None, **kw):
            seen.update(kw)
            return [["a"]], [[1.0]]

    engine.index = Probe()
    engine.retrieve(q, 10, mmr_lambda=0.25, mmr_candidates=64)
    assert seen == {"mmr_lambda": 0.25, "mmr_candidates": 64} and not engine.cache
    seen.clear()
    engine.retrieve(q, 10)
    assert seen == {} and len(engine.cache) == 1      # a plain call: today's keywords, cached


def test_evaluation_bounds_and_cli_flags():
    from rtrec_amd import evaluate_model as em
    from rtrec_amd.evaluation.offline import _mmr_candidates
    assert _mmr_candidates(100, None, None, 3000) == 0
    assert _mmr_candidates(100, 0.5, None, 3000) == 128 and _mmr_candidates(10, 0.5, None, 3000) == 100
    assert _mmr_candidates(10, 0.5, None, 60) == 60
    for kw in ((10, 1.5, None), (10, 0.5, 9), (10, 0.5, 129), (129, 0.5, None), (10, None, 50)):
        with pytest.raises(ValueError):
            _mmr_candidates(*kw, 3000)
    args = em.build_parser().parse_args([])
    assert args.mmr_lambda is None and args.mmr_candidates is None
    args = em.build_parser().parse_args(["--mmr-lambda", "0.5", "--mmr-candidates", "120"])
    assert args.mmr_lambda == 0.5 and args.mmr_candidates == 120
