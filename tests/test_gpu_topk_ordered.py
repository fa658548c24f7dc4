"""Flat-IP top-K on ROW-ORDERED corpora (tests/_ordered_corpora.py): ascending,
descending, runs, sawteeth and clustered tops, with exact integer scores, so
every comparison is np.array_equal on ids and scores against
oracle.flat_ip_search — no tolerance, no tie rule.

The candidate-buffer scans are order dependent (how full a query's region gets
depends on where the passing rows sit); rows drawn i.i.d. never fill a region
at the wrong moment. What these cases are aimed at:
  * csrc/topk_v4.h: the stretch after the LAST compaction check (a region at
    896 of 1,024 entries took 160 or 192 more; tests/test_ordered_corpora_cpu.py
    holds the count model that shows it on the mode-4 grid below);
  * csrc/topk_v3.h: scores ascending inside one 16-bit key bucket, where a
    compaction keeps everything it is allowed to (`bucket_ascending`).
The one compile-time variant of the v4 scan, RT_TOPK_V4_QS (query sets per
wave), cannot be reached from rt_flatip_topk_tuning; its budget is covered by
the static_assert next to kRoom. What the tuning can select — forced v4,
per-split thresholds (+4), no presample (+16), stride / rank — is selected
below."""
import functools

import numpy as np
import pytest
import torch

import _ordered_corpora as oc
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    yield kernels
    kernels.topk_tuning(0, 0, -1)


@pytest.fixture
def tune(K):
    """rt_flatip_topk_tuning for one test; the planner's own choice after."""
    yield K.topk_tuning
    K.topk_tuning(0, 0, -1)


@functools.lru_cache(maxsize=None)
def _multi(nx, d, nq_plan=512):
    """The multi-ordering corpus and the oracle's top-128 of every (group,
    scale) pair, computed once; a test's query j is pair j mod (6 G), and any
    k <= 128 is a prefix (no ties)."""
    x, ranks, names = oc.multi_corpus(nx, d, nq_plan=nq_plan, phase0=8 if (d < 96 and nx % 2) else 0)
    upairs = oc.cycle_pairs(len(names), 6 * len(names))
    uq = oc.queries(upairs, d)
    rs, ri = orc.flat_ip_search(uq, x, 128, nthreads=16)
    for a in (x, uq, rs, ri):  # shared by every test of the file
        a.setflags(write=False)
    return x, names, uq, rs, ri


def _dev(a, dtype):
    return torch.tensor(a).to("cuda", dtype)


def _assert_equal(gs, gi, rs, ri, what=""):
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    bad = np.nonzero((gi != ri).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[:8]}: got {gi[bad[0]][:6]} "
                           f"{gs[bad[0]][:6]} want {ri[bad[0]][:6]} {rs[bad[0]][:6]}")
    assert np.array_equal(gs, rs), what


def _check_multi(K, nx, d, dtype, ks, nq=512, nq_plan=512):
    x, names, uq, rs, ri = _multi(nx, d, nq_plan)
    idx = np.arange(nq) % uq.shape[0]
    q, xd = _dev(uq[idx], dtype), _dev(x, dtype)
    for k in ks:
        gs, gi = K.flatip_topk(q, xd, k)
        torch.cuda.synchronize()
        _assert_equal(gs, gi, rs[idx, :k], ri[idx, :k], f"nx={nx} d={d} k={k}")


# ---- 1. mode 4: external thresholds, the deterministic tail -----------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("nx", oc.MODE4_N)
def test_mode4_tail_after_last_check(K, tune, nx, d, dtype):
    """rt_flatip_topk_shard_search (the v4 scan in mode 4) on one ascending
    group: query j's threshold is the score of row nx - P_j, so exactly its
    last P_j rows pass, nothing earlier, and no compaction fires before a
    region exceeds 896 entries. P_j (oc.MODE4_P) sweeps 840 .. 1,110; the
    sizes are whole stages, then 1, 31, 32 and 97 rows into the last one, at
    the issue's 8,192+ (8 splits) and at 1,152+ (ONE split of 9-10 stages,
    where a region does receive more than 1,024 passing rows: the sizes at
    which the old check placement overflowed, see the count model). Scales
    alternate 1, 2, 4: an entry strayed in from a neighbour's region carries a
    visibly wrong score. d = 128 is the 4-stage ring, d = 64 the 3-stage one.
    Every query must return rows nx-1 .. nx-100, all valid."""
    tune(2, 0, -1)
    nq, k, off = len(oc.MODE4_P), 100, 5_000_000
    ranks = oc.ascending(nx)[:, None]
    x = oc.encode(ranks, d)
    scale = np.array([(1.0, 2.0, 4.0)[j % 3] for j in range(nq)], np.float32)
    q = oc.queries([(0, c) for c in scale], d)
    p = np.array(oc.MODE4_P)
    thr = (scale * (nx - p)).astype(np.float32)
    gs, gi = K.flatip_topk_shard_search(_dev(q, dtype), _dev(x, dtype), k, torch.from_numpy(thr).cuda(),
                                        id_offset=off)
    torch.cuda.synchronize()
    # the oracle on the thresholded set (its top 100 lie in the last 840 rows for every query)
    cut = nx - p.min()
    rs3, ri3 = orc.flat_ip_search(q[:3], x[cut:], k, id_offset=off + cut, nthreads=3)
    assert np.array_equal(ri3, np.broadcast_to(off + nx - 1 - np.arange(k), (3, k)))
    rs, ri = rs3[np.arange(nq) % 3], ri3[np.arange(nq) % 3]
    assert (gi.cpu().numpy() >= 0).all()
    _assert_equal(gs, gi, rs, ri, f"nx={nx} d={d}")
    assert np.array_equal(gs.cpu().numpy() / scale[:, None], np.broadcast_to(rs3[0], (nq, k)))


# ---- 2. v4, running and sampled thresholds -----------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 96, 64])
@pytest.mark.parametrize("nx", [24000, 30011])
@pytest.mark.parametrize("mode,stride,rank", [(2, 16, 0), (2, 1, 3), (2, 32, 32), (6, 16, 0), (18, 0, -1)],
                         ids=["running", "stride1rank3", "stride32rank32", "running_per_split", "no_presample"])
def test_v4_ordered(K, tune, mode, stride, rank, nx, d, dtype):
    """The forced v4 pair on the multi-ordering corpus, 512 queries (one block
    of queries: the last region of the last split borders the entry counts),
    k = 1, 10, 100, 128. rank 0: a running threshold from -inf, every region
    driven by compactions — the desc_then_asc runs sweep the phase at which
    the last check finds it. (1, 3): every stage sampled, the 3rd largest group
    maximum as threshold: far above the k-th score, verification fails and the
    blocks rescan. (32, 32): stage 0 of each split only — too low a threshold
    where the top sits in a skipped stage (compactions), too high where it
    sits in stage 0 (rescans). +4 (mode 6): per-split thresholds; +16 (mode
    18): the planner's sample without the presample launch.
    d = 128 is the 4-stage ring; d = 96 and 64 the 3-stage one. A 64-dim row
    holds 21 groups only: there the corpus drops sawtooth(4096) and three of
    the five clustered positions (first stage, sampled stage, skipped stage)
    in favour of 16 run phases; d = 96 (32 groups) carries every ordering and
    every clustered position on the 3-stage ring, with 22 run phases."""
    tune(mode, stride, rank)
    _check_multi(K, nx, d, dtype, (1, 10, 100, 128))


# ---- 3. v4 as the planner picks it -------------------------------------------
@pytest.mark.parametrize("nq", [128, 8192])
def test_planner_choice_ordered(K, nq):
    """No tuning, nx = 65,536 + 97, d = 128, f16, k = 100. With 128 queries
    (the shape the advisor named) the planner does NOT choose v4 — one query
    tile cannot fill the chip — and the v2 kernel runs; from 16 query tiles
    (8,192 queries) on it does: presample, corpus-wide threshold, scan, finish,
    rescue. rt_flatip_topk_shard_plan tells which. (The clustered groups are
    placed against the v4 item splits, 4,224 rows at both query counts; the
    v2 run at nq = 128 cuts its own splits, so there they are plain positions.)"""
    nx, d, k = 65536 + 97, 128, 100
    plan = K.flatip_topk_shard_plan(nq, nx, d, F16, k, 1)
    assert (plan is not None) == (nq == 8192)
    _check_multi(K, nx, d, F16, (k,), nq=nq, nq_plan=8192)


# ---- 4. v2 / v3 ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 96, 64])
@pytest.mark.parametrize("nx", [9001, 20000])
def test_v2_v3_ordered(K, tune, nx, d, dtype):
    """v4 switched off (tuning 1). Dispatch (csrc/topk_impl.h, launch_S): a
    16-bit corpus with d <= 128 runs topk_v3.h for k <= 32 (k = 10 here) and
    topk_v2.h above (k = 100, 128); the API does not report which. The
    `bucket_ascending` group is the v3 case: inside a 1,024-score key bucket
    every compaction keeps all it may and every new row passes."""
    tune(1, 0, -1)
    _check_multi(K, nx, d, dtype, (10, 32, 100, 128))


@pytest.mark.parametrize("mode", [1, 9], ids=["dense", "fused"])
@pytest.mark.parametrize("nx", [9001, 20000])
def test_f32_ordered(K, tune, nx, mode):
    """The same corpora in fp32 through rt_flatip_topk: the register-list
    kernels (k <= 32) or the score-slab pair where it applies, v2 above."""
    tune(mode, 0, -1)
    _check_multi(K, nx, 128, F32, (10, 32, 100, 128), nq=256)


# ---- 5. exclusion and id offset -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _excluded_case():
    nx, d, nq, off = 24000, 128, 192, 3_000_000
    ranks = oc.ascending(nx)[:, None]
    x = oc.encode(ranks, d)
    pairs = oc.cycle_pairs(1, nq)
    q = oc.queries(pairs, d)
    rng = np.random.default_rng(7)
    excl = [nx - 2000 + rng.choice(2000, 666, replace=False) for _ in range(nq)]
    bm = orc.exclusion_bitmap(nq, nx, excl)
    rs, ri = orc.flat_ip_search(q, x, 128, exclude_bits=bm, id_offset=off, nthreads=16)
    return x, q, excl, off, rs, ri


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mode,stride,rank", [(2, 16, 0), (2, 0, -1), (1, 0, -1)], ids=["v4_running", "v4", "v2_v3"])
def test_ordered_exclusion_and_offset(K, tune, mode, stride, rank, dtype):
    """Ascending corpus; per query a random third of the last 2,000 rows is
    excluded (for the positive scales: a third of the rows that would pass),
    with an id offset."""
    x, q, excl, off, rs, ri = _excluded_case()
    tune(mode, stride, rank)
    bits = K.exclusion_bitmap(q.shape[0], x.shape[0], excl, "cuda")
    qd, xd = _dev(q, dtype), _dev(x, dtype)
    for k in (10, 100):
        gs, gi = K.flatip_topk(qd, xd, k, exclude_bits=bits, id_offset=off)
        torch.cuda.synchronize()
        _assert_equal(gs, gi, rs[:, :k], ri[:, :k], f"k={k}")


# ---- 6. the sharded flow on one GPU ------------------------------------------
@functools.lru_cache(maxsize=None)
def _shard_case():
    nx, d, nq = 40000, 128, 256
    ranks = np.stack([oc.ascending(nx), oc.clustered_top(nx, nx - 128, 128, seed=1)], axis=1)
    x = oc.encode(ranks, d)
    # ascending under every scale (negative: the top sits in the FIRST shard), the clustered top under the positive ones
    base = [(0, c) for c in oc.SCALES] + [(1, c) for c in (1.0, 2.0, 4.0)]
    pairs = [base[j % len(base)] for j in range(nq)]
    q = oc.queries(pairs, d)
    rs, ri = orc.flat_ip_search(q, x, 100, nthreads=16)
    return x, q, pairs, rs, ri


@pytest.mark.parametrize("stride", [None, 32], ids=["library_stride", "stride32"])
@pytest.mark.parametrize("n_shards", [2, 8])
def test_sharded_flow_ordered(K, tune, n_shards, stride):
    """sample -> threshold -> search -> merge as N ranks run them (see
    test_shard_global_threshold_emulated; rtrec_amd/dist/sharded.py::
    sharded_topk_global), on an ascending plus clustered corpus of 40,000
    rows: the last shard holds the whole top-k of the positive-scale queries.
    Every merged list is full and equals the oracle.
      * the library's stride for this size (9 stages) samples a fifth of every
        10-stage split: no rank <= 32 is failure-safe, rt_topk_sample_rank says
        0 and the library searches every shard from -FLT_MAX — mode 4 with a
        running threshold, on rows that all pass;
      * stride 32 samples stage 0 of every split (a tenth): a safe rank exists,
        and for the ascending group the threshold falls inside the last shard:
        the shards below it return nothing."""
    from rtrec_amd.dist.sharded import shard_range
    x, q, pairs, rs, ri = _shard_case()
    nx, k = x.shape[0], 100
    tune(2, 0, -1)
    qd, xd = _dev(q, F16), _dev(x, F16)
    lib_stride = K.shard_sample_stride(nx)
    assert lib_stride == 9
    stride = stride or lib_stride
    tops, sampled, stages, spans = [], 0, 0, []
    for r in range(n_shards):
        b, c = shard_range(nx, n_shards, r)
        spans.append((b, c))
        top, (sa, st) = K.flatip_topk_shard_sample(qd, xd[b:b + c], k, stride)
        tops.append(top)
        sampled += sa
        stages += st
    rank = K.topk_sample_rank(k, sampled, stages)
    assert (rank > 0) == (stride == 32), (rank, sampled, stages)
    if rank > 0:
        thr = K.topk_sample_threshold(torch.stack(tops), rank)
    else:  # as sharded_topk_global does
        thr = torch.full((q.shape[0],), -3.4028234663852886e38, dtype=torch.float32, device="cuda")
    ss, ii = [], []
    for b, c in spans:
        s, i = K.flatip_topk_shard_search(qd, xd[b:b + c], k, thr, id_offset=b)
        ss.append(s)
        ii.append(i)
    ms, mi = K.topk_merge(torch.stack(ss), torch.stack(ii), k)
    torch.cuda.synchronize()
    assert (mi >= 0).all(), "a merged list is not full"
    _assert_equal(ms, mi, rs, ri, f"{n_shards} shards")
    if rank > 0:
        asc_pos = torch.tensor([g == 0 and c > 0 for g, c in pairs], device="cuda")
        for i in ii[:-1]:
            assert (i[asc_pos] < 0).all(), "a shard below the last holds rows above the threshold"
        assert (ii[-1][asc_pos] >= 0).all()


@pytest.mark.parametrize("mode", [0, 2], ids=["planner", "v4"])
def test_sharded_index_ordered(K, tune, device, mode):
    """The same corpus through ShardedFlatIPIndex (single rank) against
    HipFlatIPIndex (as test_gpu_dist.py::test_sharded_index_single_rank_matches_flat_index)
    and the oracle; forced v4 takes the corpus-wide-threshold path."""
    from rtrec_amd.dist.sharded import ShardedFlatIPIndex
    from rtrec_amd.serving.retrieval import HipFlatIPIndex
    x, q, pairs, rs, ri = _shard_case()
    tune(mode, 0, -1)
    sh = ShardedFlatIPIndex(128, device=device, storage_dtype=F16, metric="inner_product").build(x)
    flat = HipFlatIPIndex({"dimension": 128, "metric": "inner_product", "device": str(device),
                           "storage_dtype": "float16"})
    flat.build(x, [str(i) for i in range(len(x))])
    s1, i1 = sh.search_tensors(q, 100)
    s2, i2 = flat.search_tensors(q, 100)
    torch.cuda.synchronize()
    _assert_equal(s1, i1, rs, ri, "sharded index")
    _assert_equal(s2, i2, rs, ri, "flat index")


# ---- 7. the dense fp32 path ----------------------------------------------------
def test_dense_ordered_several_slabs(K):
    """topk_dense.h at its smallest multi-slab shape (test_dense_several_slabs:
    20,000 queries x 4,096 rows, d = 8) on an ascending and a clustered group:
    the score-slab GEMM + select has no order dependence."""
    nx, d, nq, k = 4096, 8, 20000, 10
    ranks = np.stack([oc.ascending(nx), oc.clustered_top(nx, 1000, 128, seed=2)], axis=1)
    x = oc.encode(ranks, d)
    upairs = oc.cycle_pairs(2, 12)
    uq = oc.queries(upairs, d)
    rs, ri = orc.flat_ip_search(uq, x, k, nthreads=4)
    idx = np.arange(nq) % 12
    gs, gi = K.flatip_topk(_dev(uq[idx], F32), _dev(x, F32), k)
    torch.cuda.synchronize()
    _assert_equal(gs, gi, rs[idx], ri[idx], "dense")
