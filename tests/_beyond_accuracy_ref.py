"""fp64 numpy restatement of the two beyond-accuracy list metrics, written from
their definitions in the PAIRWISE form (every pair i < j is visited through
the row's similarity matrix), not through the sum identity the kernel uses.
Test yardstick only.

For a row of ``preds`` the list is its non-negative entries in order; at ``k``
the first ``n = min(k, len)`` entries count.

diversity@k of a row (n >= 2): mean over pairs i < j of ``1 - ê_i·ê_j`` with
``ê = e / (‖e‖ + 1e-8)``; the result is the mean over rows with n >= 2 (0.0
without any). novelty@k: flat mean over every counted entry of every row of
``-log2(pop/total + 1e-10)``, pop = the item's count or 1 when the table does
not hold it, total = the sum of the counts held (0.0 without entries).
"""
import numpy as np


def row_list(row):
    row = np.asarray(row, np.int64)
    return row[row >= 0]


def diversity_rows(preds, emb, ks):
    """(per-row diversity fp64 [n_rows, n_k], valid bool [n_rows, n_k]); ``emb``
    is read as float64 copies of its stored values. The pair distances of a
    row are formed once and each k averages its own upper triangle."""
    e64 = np.asarray(emb, np.float64)
    ks = [int(k) for k in ks]
    vals = np.zeros((len(preds), len(ks)), np.float64)
    valid = np.zeros((len(preds), len(ks)), bool)
    for r, row in enumerate(preds):
        items = row_list(row)[:max(ks)]
        if len(items) < 2:
            continue
        x = e64[items]
        xh = x / (np.sqrt((x * x).sum(axis=1, keepdims=True)) + 1e-8)
        dist = 1.0 - xh @ xh.T
        for c, k in enumerate(ks):
            n = min(k, len(items))
            if n < 2:
                continue
            iu = np.triu_indices(n, 1)  # every pair i < j of the first n
            vals[r, c] = dist[:n, :n][iu].mean()
            valid[r, c] = True
    return vals, valid


def diversity(preds, emb, k):
    vals, valid = diversity_rows(preds, emb, [k])
    return float(vals[valid].mean()) if valid.any() else 0.0


def _terms(pop_items, pop_counts):
    table = {int(i): int(c) for i, c in zip(pop_items, pop_counts)}
    total = sum(table.values())
    return lambda it: -np.log2(table.get(int(it), 1) / total + 1e-10)


def novelty_rows(preds, pop_items, pop_counts, ks):
    """(per-row Σ terms fp64 [n_rows, n_k], per-row entry count [n_rows, n_k]);
    the popularity table comes as two arrays."""
    term = _terms(pop_items, pop_counts)
    ks = [int(k) for k in ks]
    sums = np.zeros((len(preds), len(ks)), np.float64)
    cnts = np.zeros((len(preds), len(ks)), np.int64)
    for r, row in enumerate(preds):
        t = np.array([term(it) for it in row_list(row)[:max(ks)]], np.float64)
        for c, k in enumerate(ks):
            sums[r, c] = t[:k].sum()
            cnts[r, c] = len(t[:k])
    return sums, cnts


def novelty(preds, pop_items, pop_counts, k):
    sums, cnts = novelty_rows(preds, pop_items, pop_counts, [k])
    return float(sums.sum() / cnts.sum()) if cnts.sum() else 0.0
