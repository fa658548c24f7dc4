"""Numpy fp64 restatement of the 8-bit scalar quantiser for the IVF-SQ8 tests: decode,
encode and the scores / search over probed lists that define what rt_sq8_encode,
rt_ivf_sq8_topk and HipIVFSQ8Index must return. No Faiss, nothing from the reference."""
import numpy as np


def decode(codes, lo, step):
    return np.asarray(lo, np.float64) + (np.asarray(codes, np.float64) + 0.5) * np.asarray(step, np.float64)


def encode(rows, lo, inv_step, centroids=None, assign=None):
    """(uint8 [n, d], fp64 t [n, d]): t = (r - lo) inv_step, r the row or, where assign is
    inside [0, nlist), ``row - centroids[assign]``; code 255 for t >= 255, floor(t) for t > 0, else 0."""
    r = np.asarray(rows, np.float64).copy()
    if centroids is not None:
        a = np.asarray(assign)
        ok = (a >= 0) & (a < len(centroids))
        r[ok] -= np.asarray(centroids, np.float64)[a[ok]]
    t = (r - np.asarray(lo, np.float64)) * np.asarray(inv_step, np.float64)
    return np.where(t >= 255, 255, np.where(t > 0, np.floor(t), 0)).astype(np.uint8), t


def scores(queries, codes, lo, step, list_offsets, row_pos, probes, bias, exclude=None):
    """Per query: (positions, scores, magnitudes) fp64 of every row of the probed lists that is
    not excluded (``exclude`` bool [nq, n] by original position; a probe outside [0, nlist) names
    no list). magnitude = |bias| + sum |q_j mid_j| + sum |q_j step_j| code_j."""
    q = np.asarray(queries, np.float64)
    lo, step = np.asarray(lo, np.float64), np.asarray(step, np.float64)
    mid = lo + 0.5 * step
    nlist = len(list_offsets) - 1
    out = []
    for i, pr in enumerate(np.asarray(probes)):
        pos, sc, mg = [np.zeros(0, np.int64)], [np.zeros(0)], [np.zeros(0)]
        for p, l in enumerate(pr):
            if not 0 <= l < nlist:
                continue
            sl = slice(list_offsets[l], list_offsets[l + 1])
            c = codes[sl].astype(np.float64)
            b = 0.0 if bias is None else float(bias[i, p])
            pos.append(row_pos[sl].astype(np.int64))
            sc.append(b + q[i] @ mid + c @ (q[i] * step))
            mg.append(abs(b) + np.abs(q[i] * mid).sum() + c @ np.abs(q[i] * step))
        pos, sc, mg = np.concatenate(pos), np.concatenate(sc), np.concatenate(mg)
        if exclude is not None:
            keep = ~exclude[i][pos]
            pos, sc, mg = pos[keep], sc[keep], mg[keep]
        out.append((pos, sc, mg))
    return out


def search(queries, codes, lo, step, list_offsets, row_pos, probes, bias, k, exclude=None):
    """(scores fp64 [nq, k], positions int64 [nq, k]) in (score desc, position asc) order over the
    probed lists; unfilled slots (-inf, -1)."""
    nq = len(queries)
    S, I = np.full((nq, k), -np.inf), np.full((nq, k), -1, np.int64)
    for i, (pos, sc, _) in enumerate(scores(queries, codes, lo, step, list_offsets, row_pos, probes, bias, exclude)):
        order = np.lexsort((pos, -sc))[:k]
        S[i, :len(order)], I[i, :len(order)] = sc[order], pos[order]
    return S, I
