"""Numpy fp64 restatement of product quantisation for the IVF-PQ tests: the
encode (argmin, lowest index on ties), the lookup tables and the ADC search
over probed lists that defines what rt_ivf_pq_topk and HipIVFPQIndex must
return. No Faiss, nothing from the reference."""
import numpy as np


def encode(rows, codebooks, centroids=None, assign=None):
    """(uint8 [n, M], fp64 distances [n, M, 256]): per subspace the nearest codeword to the row —
    to ``row - centroids[assign]`` where assign is inside [0, nlist) — the lowest index on ties."""
    r = np.asarray(rows, np.float64).copy()
    if centroids is not None:
        a = np.asarray(assign)
        ok = (a >= 0) & (a < len(centroids))
        r[ok] -= np.asarray(centroids, np.float64)[a[ok]]
    cb = np.asarray(codebooks, np.float64)
    M, _, dsub = cb.shape
    dist = ((r.reshape(len(r), M, 1, dsub) - cb[None]) ** 2).sum(axis=3)
    return np.argmin(dist, axis=2).astype(np.uint8), dist


def tables(queries, codebooks):
    """lut [nq, M, 256] fp64 and the same sums over absolute products."""
    cb = np.asarray(codebooks, np.float64)
    M, _, dsub = cb.shape
    q = np.asarray(queries, np.float64).reshape(len(queries), M, 1, dsub)
    return (q * cb[None]).sum(axis=3), np.abs(q * cb[None]).sum(axis=3)


def adc_scores(queries, codes, codebooks, list_offsets, row_pos, probes, bias, exclude=None):
    """Per query: (positions, scores, magnitudes) fp64 of every row of the probed lists that is
    not excluded (``exclude`` bool [nq, n] by original position; a probe outside [0, nlist) names
    no list). magnitude = |bias| + sum |products|, what the fp32 rounding bound scales with."""
    lut, mag = tables(queries, codebooks)
    M = codes.shape[1]
    nlist = len(list_offsets) - 1
    out = []
    for q, pr in enumerate(np.asarray(probes)):
        pos, sc, mg = [], [], []
        for p, l in enumerate(pr):
            if not 0 <= l < nlist:
                continue
            sl = slice(list_offsets[l], list_offsets[l + 1])
            c = codes[sl].astype(np.int64)
            b = 0.0 if bias is None else float(bias[q, p])
            pos.append(row_pos[sl].astype(np.int64))
            sc.append(b + lut[q, np.arange(M), c].sum(axis=1))
            mg.append(abs(b) + mag[q, np.arange(M), c].sum(axis=1))
        pos = np.concatenate(pos) if pos else np.zeros(0, np.int64)
        sc = np.concatenate(sc) if sc else np.zeros(0)
        mg = np.concatenate(mg) if mg else np.zeros(0)
        if exclude is not None:
            keep = ~exclude[q][pos]
            pos, sc, mg = pos[keep], sc[keep], mg[keep]
        out.append((pos, sc, mg))
    return out


def adc_search(queries, codes, codebooks, list_offsets, row_pos, probes, bias, k, exclude=None):
    """(scores fp64 [nq, k], positions int64 [nq, k]) in (score desc, position asc)
    order over the probed lists; unfilled slots (-inf, -1)."""
    nq = len(queries)
    S = np.full((nq, k), -np.inf)
    I = np.full((nq, k), -1, np.int64)
    for q, (pos, sc, _) in enumerate(adc_scores(queries, codes, codebooks, list_offsets, row_pos, probes, bias,
                                                exclude)):
        order = np.lexsort((pos, -sc))[:k]
        S[q, :len(order)], I[q, :len(order)] = sc[order], pos[order]
    return S, I


def check_topk(got_s, got_i, cand, k, tol_factor):
    """One query, ``cand`` = its adc_scores entry: every returned id is eligible and distinct, its
    score within tol of the fp64 score, no row left out scores above the k-th returned plus tol."""
    pos, sc, mg = cand
    where = {int(p): i for i, p in enumerate(pos)}
    n_want = min(k, len(pos))
    ids = [int(i) for i in got_i if i >= 0]
    assert len(ids) == n_want and len(set(ids)) == n_want, (len(ids), n_want)
    assert all(i in where for i in ids), "an id outside the probed, non-excluded rows"
    idx = np.array([where[i] for i in ids], np.int64)
    tol = tol_factor * mg
    assert np.all(np.abs(got_s[:n_want].astype(np.float64) - sc[idx]) <= tol[idx])
    assert np.all(got_i[n_want:] == -1)
    if n_want and len(pos) > n_want:
        out = np.ones(len(pos), bool)
        out[idx] = False
        kth = float(got_s[n_want - 1])
        assert np.all(sc[out] <= kth + tol[out])   # kth is the device's own fp32 score
