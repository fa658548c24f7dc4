"""The ordered-corpus fixtures (tests/_ordered_corpora.py) are what they claim
to be — exact in fp32, f16 and bf16, scores equal to the integer ranks, the
oracle's top-k equal to the closed form — and the count model of the v4 scan
shows that the mode-4 grid of tests/test_gpu_topk_ordered.py overflows a
candidate region under the OLD placement of the compaction checks and cannot
under the new one. No GPU: this is the evidence that the GPU test would have
failed before the fix, without running the code that wrote out of bounds."""
import numpy as np
import pytest
import torch

import _ordered_corpora as oc
from oracle import flat_ip as orc


@pytest.fixture(scope="module", params=[(128, 3001), (96, 1500), (64, 2777)], ids=lambda p: f"d{p[0]}")
def corpus(request):
    d, nx = request.param
    x, ranks, names = oc.multi_corpus(nx, d)
    pairs = oc.cycle_pairs(len(names), 6 * len(names))
    return d, nx, x, ranks, names, pairs, oc.queries(pairs, d)


def test_groups_fill_the_row(corpus):
    d, nx, x, ranks, names, pairs, q = corpus
    assert len(names) == oc.n_groups(d) == ranks.shape[1]
    assert {"ascending", "sawtooth128", "bucket_ascending", "top_ragged_end",
            "top_split_boundary"} <= set(names)
    runs = sorted(int(n[3:]) for n in names if n.startswith("run"))
    assert len(runs) >= 16 and runs[-1] - runs[0] >= 240 and set(np.diff(runs)) <= {8, 16}
    for g in range(ranks.shape[1]):  # no ties inside a group
        assert np.unique(ranks[:, g]).size == nx, names[g]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_exact_in_every_dtype(corpus, dtype):
    d, nx, x, ranks, names, pairs, q = corpus
    for a in (x, q):
        t = torch.from_numpy(a)
        assert torch.equal(t.to(dtype).to(torch.float32), t)


def test_scores_are_the_ranks(corpus):
    d, nx, x, ranks, names, pairs, q = corpus
    s = x.astype(np.float64) @ q.astype(np.float64).T
    want = np.stack([c * ranks[:, g] for g, c in pairs], axis=1).astype(np.float64)
    assert np.array_equal(s, want)
    assert np.abs(s).max() < 2 ** 24
    # every partial sum is an integer below 2^24 too: fp32 in any order agrees
    assert np.array_equal((x @ q.T).astype(np.float64), want)
    assert np.array_equal((x[:, ::-1] @ q[:, ::-1].T).astype(np.float64), want)


@pytest.mark.parametrize("k", [1, 10, 128])
def test_oracle_equals_closed_form(corpus, k):
    d, nx, x, ranks, names, pairs, q = corpus
    rs, ri = orc.flat_ip_search(q, x, k, nthreads=4)
    cs, ci = oc.closed_form_topk(ranks, pairs, k)
    assert np.array_equal(ri, ci)
    assert np.array_equal(rs, cs)


def test_oracle_equals_closed_form_excluded_offset():
    nx, d = 2500, 64
    ranks = oc.ascending(nx)[:, None]
    pairs = [(0, c) for c in oc.SCALES]
    rng = np.random.default_rng(0)
    excl = [nx - 2000 + rng.choice(2000, 666, replace=False) for _ in pairs]
    x, q = oc.encode(ranks, d), oc.queries(pairs, d)
    rs, ri = orc.flat_ip_search(q, x, 100, exclude_bits=orc.exclusion_bitmap(len(pairs), nx, excl),
                                id_offset=10 ** 6, nthreads=2)
    cs, ci = oc.closed_form_topk(ranks, pairs, 100, exclude=excl, id_offset=10 ** 6)
    assert np.array_equal(ri, ci) and np.array_equal(rs, cs)


def test_clustered_top_is_contiguous():
    r = oc.clustered_top(5000, 1234, 128, seed=3)
    assert np.array_equal(np.sort(np.argsort(-r)[:128]), np.arange(1234, 1234 + 128))
    assert np.unique(r).size == 5000


def test_v4_splits_restated():
    """Spot values of csrc/topk_api.hip::plan_v4 (forced): < 16 stages stay in
    one split; the mode-4 sizes of the issue are cut into 8."""
    assert oc.v4_splits(271, 1152) == (1152, 1)
    assert oc.v4_splits(271, 1249) == (1280, 1)
    assert oc.v4_splits(271, 8192) == (1024, 8)
    assert oc.v4_splits(271, 8193) == (1152, 8)
    assert oc.v4_splits(512, 24000) == (1536, 16)
    assert oc.v4_splits(65536, 125000) == (62592, 2)


# ---- the count model ----
def test_count_model_by_hand():
    """A 9-stage split whose last 1,040 rows pass (first_pass = 112)."""
    # ring 4, late set, old: end of stage 7 sees 8 * 128 - 32 - 112 = 880 <= 896,
    # then five more sub-tiles: 880 + 160 = 1,040 > 1,024
    assert oc.count_model(1152, 112, 4, False, True) == (1040, 880, False)
    # new: the end of stage 8 sees 1,008 and compacts; the flush adds <= 32
    assert oc.count_model(1152, 112, 4, True, True) == (1008, 1008, True)
    # the other set stores at once: 896 at the end of stage 7, 128 more: full, not over
    assert oc.count_model(1152, 128, 4, False, False) == (1024, 896, False)
    # ring 3, old: both sets overflow (the check sits one sub-tile earlier)
    assert oc.count_model(1152, 112, 3, False, False) == (1040, 880, False)
    assert oc.count_model(1152, 80, 3, False, True) == (1072, 880, False)
    for ring in (3, 4):
        for late in (False, True):
            assert oc.count_model(1152, 0, ring, True, late)[0] <= oc.V4_CAP


@pytest.mark.parametrize("ring", [4, 3])
def test_mode4_grid_overflows_old_placement_only(ring):
    """On the grid of the GPU test (query j < 271 passing its last 840 + j
    rows, the rest the same tails rotated): under the old placement some queries end above the region's
    1,024 entries although every check saw <= 896 (no compaction: the counts
    are exact) — entries written into the next query's region, or past the
    buffer. Under the new placement no region can exceed its capacity, however
    little a compaction drops."""
    nq = len(oc.MODE4_P)
    over = []
    for nx in oc.MODE4_N:
        for j, p in enumerate(oc.MODE4_P):
            late = (j % 64) >= 32
            peak, seen, compacted = oc.mode4_peak(nq, nx, p, ring, False, late)
            if peak > oc.V4_CAP and seen <= oc.V4_ROOM:
                assert not compacted
                over.append((nx, j, peak))
            assert oc.mode4_peak(nq, nx, p, ring, True, late)[0] <= oc.V4_CAP, (nx, j)
    assert over, "the grid never overflows the old placement"
    # whole stages, and the 97-row tail (a tail of r rows shortens the stretch after
    # the last check to r + 32 or r + 64 rows: 1, 31 and 32 stay inside the budget)
    assert {nx for nx, _, _ in over} == {1152, 1249}
    worst = max(pk for _, _, pk in over)
    # the late set's tail: NSUB + 1 (ring 4) or NSUB + 2 (ring 3) sub-tiles after the last check
    assert worst == oc.V4_ROOM + (160 if ring == 4 else 192)
    if ring == 3:  # there the other set overflows as well
        assert any((j % 64) < 32 for _, j, _ in over)
    # at the sizes the issue names the planner cuts 8 splits: no region can overflow
    for nx in oc.MODE4_N_ISSUE:
        assert all(oc.mode4_peak(nq, nx, p, ring, False, True)[0] <= oc.V4_CAP for p in oc.MODE4_P)


def test_new_placement_budget_exhaustive():
    """Any split length up to 20 stages, any first passing row on an 8-row
    grid, both rings, both sets: the new placement keeps every region within
    capacity — the static_assert of csrc/topk_v4.h, by enumeration."""
    for rows in list(range(1, 2561, 97)) + [128, 1024, 1152, 2560]:
        for first in range(0, rows, 8):
            for ring in (3, 4):
                for late in (False, True):
                    assert oc.count_model(rows, first, ring, True, late)[0] <= oc.V4_CAP


@pytest.mark.parametrize("k", [1, 10, 32])
def test_v3_bucket_model_old_keep_overflows(k):
    """Scores ascending inside 16-bit key buckets (bucket_ascending): with the
    compaction allowed to keep 448 of a query's 512 entries a lane half passes
    its 256 (k, k + 128, ... survivors: the one in (384, 448] is kept whole and
    takes a stage of appends on top); keeping at most 352 it cannot, wherever
    the bucket boundary falls."""
    old = [oc.v3_bucket_model(4096, b, k, oc.V3_KEEP_OLD) for b in range(0, 2049, 32)]
    new = [oc.v3_bucket_model(4096, b, k, oc.V3_KEEP) for b in range(0, 2049, 32)]
    assert max(old) > oc.V3_HALF
    assert max(new) <= oc.V3_HALF
