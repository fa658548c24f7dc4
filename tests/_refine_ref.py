"""Numpy fp64 restatement of rt_refine_topk for the refine tests: decode the store,
dot, drop absent ids, sort by (score desc, position asc, candidate index asc), pad."""
from collections import Counter

import numpy as np


def decode(store, lo=None, step=None):
    """fp64 rows of a store: the rows themselves, or lo + (code + 0.5) step of SQ8 codes."""
    x = np.asarray(store, np.float64)
    return x if lo is None else np.asarray(lo, np.float64) + (x + 0.5) * np.asarray(step, np.float64)


def refine(queries, cand_ids, rows, k):
    """(scores fp64 [nq, k], positions [nq, k], per query (positions, scores, sum |q_j x_j|) of its
    present candidates); unfilled slots (-inf, -1)."""
    q = np.asarray(queries, np.float64)
    S, I, cands = np.full((len(q), k), -np.inf), np.full((len(q), k), -1, np.int64), []
    for i, ids in enumerate(np.asarray(cand_ids)):
        idx = np.flatnonzero((ids >= 0) & (ids < len(rows)))
        pos = ids[idx]
        sc, mg = rows[pos] @ q[i], np.abs(rows[pos] * q[i]).sum(axis=1)
        order = np.lexsort((idx, pos, -sc))[:k]
        S[i, :len(order)], I[i, :len(order)] = sc[order], pos[order]
        cands.append((pos, sc, mg))
    return S, I, cands


def check(got_s, got_i, cand, k, tol_factor):
    """One query against its ``refine`` entry, for inputs that round: present candidates only (a
    duplicate as often as given), scores within tol_factor * sum |q_j x_j| of fp64, (score desc,
    position asc) order, pads after, no candidate left out above the last returned plus tol."""
    pos, sc, mg = cand
    n = min(k, len(pos))
    assert np.all(got_i[:n] >= 0) and np.all(got_i[n:] == -1) and np.all(got_s[n:] == -np.finfo(np.float32).max)
    left = Counter(pos.tolist()) - Counter(got_i[:n].tolist())
    assert sum(left.values()) == len(pos) - n, "a returned position that is no present candidate"
    ref = {int(p): (s, tol_factor * m) for p, s, m in zip(pos, sc, mg)}
    assert all(abs(float(s) - ref[int(i)][0]) <= ref[int(i)][1] for s, i in zip(got_s[:n], got_i[:n]))
    pairs = list(zip(-got_s[:n], got_i[:n]))
    assert pairs == sorted(pairs)
    assert all(ref[p][0] <= float(got_s[n - 1]) + ref[p][1] for p in left)
