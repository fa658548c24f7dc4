"""Diversity and novelty of recommendation lists on the GPU (rt_list_metrics,
rt_list_metrics_reduce, rtrec_amd.evaluation.compute_diversity /
compute_novelty / list_metrics_tensors, evaluate_model.beyond_accuracy).

Yardsticks: the reference's own float64 values (golden beyond_accuracy.npz)
and the pairwise fp64 restatement of tests/_beyond_accuracy_ref.py, which
tests/test_beyond_accuracy_cpu.py ties to the golden.

Tolerances (absolute): diversity 1e-10 — after the division by n(n-1) the fp64
rounding of Σ ê, Σ ‖ê‖² and ‖Σ ê‖² is a small multiple of (n + d)·2⁻⁵³, at
most ~1e-13 at n = 130, d = 1024; 1e-10 still catches any error of method
(eps placement, q = n, an off-by-one at a k boundary). Novelty 1e-9 — terms
are at most 33.3 and a sequential fp64 sum over 130,000 entries is bounded by
130,000 · 2⁻⁵³ · 33.3 ≈ 5e-10.
"""
import ctypes

import numpy as np
import pytest
import torch

import _beyond_accuracy_ref as ref

pytestmark = pytest.mark.gpu

DIV_TOL, NOV_TOL = 1e-10, 1e-9
N = 300
KS = [1, 2, 3, 10, 63, 64, 65, 100, 128]
LIST_LENS = [1, 2, 63, 64, 65, 100, 130]
ROW_COUNTS = [1, 3, 4, 5]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
GRID = [("fp32", d) for d in (4, 20, 64, 128, 130, 256, 1024)] + \
       [(t, d) for t in ("fp16", "bf16") for d in (64, 128, 256)]
N_KINDS = 12


def make_table(d, dtype, seed):
    """[N, d] in ``dtype`` plus the float64 copy of its stored values. Row 0 is
    all zero (distance 1 to everything), row 1 has norm 1e-6 (the eps moves ê
    by 1 %), rows 150.. are tightly clustered around one direction."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((N, d))
    t *= rng.uniform(0.1, 3.0, (N, 1)) / np.linalg.norm(t, axis=1, keepdims=True)
    common = rng.standard_normal(d)
    t[150:] = 0.05 * t[150:] + common / np.linalg.norm(common)
    t[0] = 0.0
    t[1] = 0.0
    t[1, :min(4, d)] = 1e-6 / np.sqrt(min(4, d))
    stored = torch.from_numpy(t).to(dtype)
    return stored, stored.to(torch.float64).numpy()


def make_lists(n_rows, list_len, first_kind, rng):
    """Row r is of kind (first_kind + r) % N_KINDS: 0 full list, 1 trailing pads,
    2 all pads, 3 one item, 4 a -1 in the middle, 5 a repeated item, 6 holds the
    zero row, 7 holds the norm-1e-6 row, 8 drawn from the clustered rows, the
    rest drawn with replacement."""
    L = list_len
    out = np.full((n_rows, L), -1, np.int64)
    for r in range(n_rows):
        kind = (first_kind + r) % N_KINDS
        full = rng.choice(np.arange(2, N), L, replace=False)
        if kind == 0:
            out[r] = full
        elif kind == 1:
            out[r, :(L + 1) // 2] = full[:(L + 1) // 2]
        elif kind == 2:
            pass
        elif kind == 3:
            out[r, 0] = full[0]
        elif kind == 4:
            out[r] = full
            out[r, L // 2] = -1
        elif kind == 5:
            out[r] = full
            out[r, -1] = full[0]
        elif kind == 6:
            out[r] = full
            out[r, min(1, L - 1)] = 0
        elif kind == 7:
            out[r] = full
            out[r, 0] = 1
        elif kind == 8:
            out[r] = rng.choice(np.arange(150, N), L, replace=False)
        else:
            out[r] = rng.integers(0, N, L)
    return out


# the popularity table holds ids below 200 except every seventh: ids from 200 on
# lie past the self-information table and take the default
POP_ITEMS = np.array([i for i in range(200) if i % 7 != 6], np.int64)
POP_COUNTS = np.random.default_rng(5).integers(1, 5000, POP_ITEMS.size).astype(np.int64)


def _info(device):
    from rtrec_amd.evaluation import self_information
    info, default = self_information({int(i): int(c) for i, c in zip(POP_ITEMS, POP_COUNTS)})
    assert info.numel() < N  # the default path is exercised
    return info.to(device), default


def check_case(device, emb_dev, emb64, lists, info, default, what):
    from rtrec_amd import kernels
    preds = torch.from_numpy(lists).to(device)
    div, valid, nov_sum, nov_cnt, summary = kernels.list_metrics(preds, KS, emb=emb_dev, info=info,
                                                                 default_info=default)
    torch.cuda.synchronize()
    want_div, want_valid = ref.diversity_rows(lists, emb64, KS)
    want_sum, want_cnt = ref.novelty_rows(lists, POP_ITEMS, POP_COUNTS, KS)
    got_div, got_valid = div.cpu().numpy(), valid.cpu().numpy().astype(bool)
    s = summary.cpu().numpy()
    assert np.array_equal(got_valid, want_valid), what
    err_row = np.abs(got_div - want_div).max() if got_div.size else 0.0
    rows_k = want_valid.sum(axis=0)
    want_mean = np.array([want_div[want_valid[:, c], c].mean() if rows_k[c] else 0.0 for c in range(len(KS))])
    err_mean = np.abs(s[0] - want_mean).max()
    ent = want_cnt.sum(axis=0)
    want_nov = np.array([want_sum[:, c].sum() / ent[c] if ent[c] else 0.0 for c in range(len(KS))])
    err_nsum = np.abs(nov_sum.cpu().numpy() - want_sum).max()
    err_nov = np.abs(s[2] - want_nov).max()
    print(f"{what}: diversity per-row err {err_row:.2e} mean err {err_mean:.2e}; "
          f"novelty per-row sum err {err_nsum:.2e} mean err {err_nov:.2e}")
    assert err_row <= DIV_TOL and err_mean <= DIV_TOL, what
    assert np.array_equal(s[1], rows_k.astype(np.float64)), what
    assert np.array_equal(nov_cnt.cpu().numpy(), want_cnt), what
    assert np.array_equal(s[3], ent.astype(np.float64)), what
    assert err_nsum <= NOV_TOL and err_nov <= NOV_TOL, what


def test_golden_reference_float64(device, golden):
    from rtrec_amd.evaluation import compute_diversity, compute_novelty
    g = golden("beyond_accuracy")
    recs = {r: [int(x) for x in row if x >= 0] for r, row in enumerate(g["lists"])}
    pop = {int(i): int(c) for i, c in zip(g["pop_items"], g["pop_counts"])}
    for name in ("table", "clustered"):
        for form in ("numpy", "device tensor"):
            emb = g[name] if form == "numpy" else torch.from_numpy(g[name]).to(device)
            for i, k in enumerate(g["k_values"]):
                got = compute_diversity(recs, emb, k=int(k))
                print(f"diversity {name} ({form}) k={k}: {got:.17g} vs {g['div64_' + name][i]:.17g} "
                      f"err {abs(got - g['div64_' + name][i]):.2e}")
                assert isinstance(got, float) and abs(got - g["div64_" + name][i]) <= DIV_TOL
    for i, k in enumerate(g["k_values"]):
        got = compute_novelty(recs, pop, k=int(k))
        print(f"novelty k={k}: {got:.17g} vs {g['novelty'][i]:.17g} err {abs(got - g['novelty'][i]):.2e}")
        assert isinstance(got, float) and abs(got - g["novelty"][i]) <= NOV_TOL


@pytest.mark.parametrize("tname,d", GRID, ids=[f"{t}-d{d}" for t, d in GRID])
def test_dispatch_grid_vs_restatement(device, tname, d):
    """Every list length × every small row count for one (dtype, d): the kinds of
    make_lists rotate through the cases so each (dtype, d) meets all of them."""
    emb, emb64 = make_table(d, DTYPES[tname], seed=d)
    emb_dev = emb.to(device)
    info, default = _info(device)
    rng = np.random.default_rng(1000 + d)
    kind = 0
    seen = set()
    for L in LIST_LENS:
        for n_rows in ROW_COUNTS:
            lists = make_lists(n_rows, L, kind, rng)
            seen |= {(kind + r) % N_KINDS for r in range(n_rows)}
            kind = (kind + n_rows) % N_KINDS
            check_case(device, emb_dev, emb64, lists, info, default, f"{tname} d={d} L={L} rows={n_rows}")
    assert seen == set(range(N_KINDS))


@pytest.mark.parametrize("tname,d,L", [("fp32", 64, 100), ("fp32", 20, 65), ("bf16", 128, 130)])
def test_thousand_rows_reduce_stride_loop(device, tname, d, L):
    emb, emb64 = make_table(d, DTYPES[tname], seed=7 * d)
    info, default = _info(device)
    lists = make_lists(1000, L, 0, np.random.default_rng(d + L))
    check_case(device, emb.to(device), emb64, lists, info, default, f"{tname} d={d} L={L} rows=1000")


@pytest.mark.parametrize("tname,d,pad,shift", [("fp32", 64, 16, 0), ("fp32", 64, 0, 1), ("fp32", 1024, 4, 1),
                                               ("fp32", 130, 2, 0), ("fp16", 64, 8, 0), ("fp16", 64, 0, 1),
                                               ("bf16", 256, 0, 3)])
def test_strided_and_unaligned_tables(device, tname, d, pad, shift):
    """A row-strided view keeps the 16-byte loads when the stride allows; a base
    pointer or stride off the 16-byte grid takes the element-load path."""
    emb, emb64 = make_table(d, DTYPES[tname], seed=3 * d + pad)
    buf = torch.zeros(N * (d + pad) + shift + 8, dtype=emb.dtype, device=device)
    view = torch.as_strided(buf, (N, d), (d + pad, 1), storage_offset=shift)
    view.copy_(emb.to(device))
    assert view.stride(0) == d + pad and (view.data_ptr() - buf.data_ptr()) == shift * emb.element_size()
    info, default = _info(device)
    lists = make_lists(12, 100, 0, np.random.default_rng(d))
    check_case(device, view, emb64, lists, info, default, f"{tname} d={d} ld={d + pad} shift={shift}")


def test_two_calls_are_bit_equal(device):
    from rtrec_amd import kernels
    emb, _ = make_table(64, torch.float32, seed=11)
    emb = emb.to(device)
    info, default = _info(device)
    preds = torch.from_numpy(make_lists(1000, 100, 0, np.random.default_rng(12))).to(device)
    a = kernels.list_metrics(preds, KS, emb=emb, info=info, default_info=default)
    b = kernels.list_metrics(preds, KS, emb=emb, info=info, default_info=default)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        if x.dtype == torch.float64:  # bit for bit, not just ==
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_id_past_the_table_is_counted_not_read(device):
    from rtrec_amd import native
    from rtrec_amd.evaluation import compute_diversity, list_metrics_tensors
    emb, emb64 = make_table(64, torch.float32, seed=13)
    emb_dev = emb.to(device)
    lists = make_lists(5, 10, 0, np.random.default_rng(14))
    lists[0, 3] = N
    recs = {r: [int(x) for x in row if x >= 0] for r, row in enumerate(lists)}
    with pytest.raises(IndexError):
        compute_diversity(recs, emb_dev, k=10)
    with pytest.raises(IndexError):
        compute_diversity(recs, emb64.astype(np.float32), k=10)
    preds = torch.from_numpy(lists).to(device)
    with pytest.raises(IndexError):
        list_metrics_tensors(preds, [10], item_embeddings=emb_dev)
    # the C entry: the id is counted once and left out of its row's list
    div = torch.empty((5, 1), dtype=torch.float64, device=device)
    valid = torch.empty((5, 1), dtype=torch.int32, device=device)
    oob = torch.zeros(1, dtype=torch.int32, device=device)
    native.call("rt_list_metrics", native.ptr(preds), 5, 10, native.ptr(emb_dev), native.RT_F32, N, 64, 64, None, 0,
                0.0, (ctypes.c_int32 * 1)(10), 1, native.ptr(div), native.ptr(valid), None, None, native.ptr(oob),
                native.stream_of(preds))
    torch.cuda.synchronize()
    assert int(oob.item()) == 1
    without = lists.copy()
    without[0, 3] = -1
    want, want_valid = ref.diversity_rows(without, emb64, [10])
    assert np.array_equal(valid.cpu().numpy().astype(bool), want_valid)
    assert np.abs(div.cpu().numpy() - want).max() <= DIV_TOL


def test_tensor_path_equals_dict_path(device, golden):
    from rtrec_amd.evaluation import compute_diversity, compute_novelty, list_metrics_tensors, self_information
    g = golden("beyond_accuracy")
    recs = {r: [int(x) for x in row if x >= 0] for r, row in enumerate(g["lists"])}
    pop = {int(i): int(c) for i, c in zip(g["pop_items"], g["pop_counts"])}
    emb = torch.from_numpy(g["clustered"]).to(device)
    info, default = self_information(pop)
    ks = [int(k) for k in g["k_values"]]
    res = list_metrics_tensors(torch.from_numpy(g["lists"]).to(device), ks, item_embeddings=emb,
                               item_info=info.to(device), default_info=default)
    assert res.per_row_diversity.is_cuda and res.diversity_valid.is_cuda
    assert res.per_row_diversity.shape == (40, 3) and res.diversity_valid.shape == (40, 3)
    lens = (g["lists"] >= 0).sum(axis=1)
    for k in ks:
        assert abs(res.diversity[k] - compute_diversity(recs, emb, k=k)) <= DIV_TOL
        assert abs(res.novelty[k] - compute_novelty(recs, pop, k=k)) <= NOV_TOL
        assert res.diversity_rows[k] == int((lens >= 2).sum())
        assert res.novelty_entries[k] == int(np.minimum(lens, k).sum())
    only_div = list_metrics_tensors(torch.from_numpy(g["lists"]).to(device), ks, item_embeddings=emb)
    assert only_div.novelty == {} and only_div.diversity == res.diversity


def test_cli_step_beyond_accuracy(device):
    """evaluate_model.beyond_accuracy on a randomly initialised model: equal to
    the restatement over the model's own item embeddings and the bincount
    popularity of the training interactions."""
    from rtrec_amd.evaluate_model import beyond_accuracy
    from rtrec_amd.evaluation import generate_recommendations
    from rtrec_amd.training.utils import create_two_tower_model_for_training
    torch.manual_seed(3)
    model = create_two_tower_model_for_training(3, 20, {"embedding_dim": 32, "hidden_layers": [64, 32],
                                                        "dropout_rate": 0.0, "temperature": 0.05})
    model.to(device).eval()
    rng = np.random.default_rng(4)
    n_items, n_users = 200, 50
    uf = rng.standard_normal((n_users, 3)).astype(np.float32)
    mf = rng.random((n_items, 20)).astype(np.float32)
    train_items = {u: rng.choice(n_items, 15, replace=False).tolist() for u in range(n_users)}
    train_idx = rng.choice([i for i in range(n_items) if i % 9], 3000)  # every ninth item never seen in training
    _, ids = generate_recommendations(model, list(range(n_users)), train_items, uf, mf, top_k=20,
                                      device=str(device), return_tensors=True)
    assert ids.is_cuda and ids.shape == (n_users, 20)
    got = beyond_accuracy(model, ids, mf, train_idx)
    with torch.no_grad():
        emb = model.get_item_embeddings({"numerical": torch.from_numpy(mf).to(device), "categorical": {}})
    assert emb.shape == (n_items, 32)
    counts = np.bincount(train_idx, minlength=n_items)
    held = np.nonzero(counts)[0]
    lists = ids.cpu().numpy()
    want_div = ref.diversity(lists, emb.double().cpu().numpy(), 10)
    want_nov = ref.novelty(lists, held, counts[held], 10)
    print(f"diversity@10 {got['diversity@10']:.17g} vs {want_div:.17g}; novelty@10 {got['novelty@10']:.17g} "
          f"vs {want_nov:.17g}")
    assert set(got) == {"diversity@10", "novelty@10"}
    assert abs(got["diversity@10"] - want_div) <= DIV_TOL
    assert abs(got["novelty@10"] - want_nov) <= NOV_TOL
