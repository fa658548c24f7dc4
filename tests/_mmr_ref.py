"""fp64 reference of the MMR re-rank (rt_mmr_rerank) for the tests.

``rows_by_pos`` maps an ORIGINAL position to its stored row: a 2-D array (row p
is position p; a row of NaNs = the position has no stored row) or a dict
``{position: row}``. A candidate is absent if its id is negative, names no
position, or the position has no row; an absent candidate is never chosen.

    obj(i) = lam * score_i - (1 - lam) * m_i,   m_i = max over the chosen j of sim(i, j)

with m_i = 0 while nothing is chosen, ties to the LOWEST candidate index, and
sim the inner product (``normalize`` false) or the cosine (true; a zero row has
similarity 0 to everything) of the stored rows, everything in fp64.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def _row(rows_by_pos, pid):
    pid = int(pid)
    if pid < 0:
        return None
    if isinstance(rows_by_pos, dict):
        r = rows_by_pos.get(pid)
        return None if r is None else np.asarray(r, dtype=np.float64)
    if pid >= len(rows_by_pos):
        return None
    r = np.asarray(rows_by_pos[pid], dtype=np.float64)
    return None if np.isnan(r).any() else r


def _setup(scores, ids, rows_by_pos, lam, normalize):
    scores = np.asarray(scores, dtype=np.float64).ravel()
    ids = np.asarray(ids, dtype=np.int64).ravel()
    assert scores.shape == ids.shape
    rows = [_row(rows_by_pos, p) for p in ids]
    present = np.array([r is not None for r in rows], dtype=bool)
    d = next((len(r) for r in rows if r is not None), 1)
    mat = np.zeros((len(ids), d), dtype=np.float64)
    for i, r in enumerate(rows):
        if r is not None:
            mat[i] = r
    sq = (mat * mat).sum(axis=1)
    sim = mat @ mat.T
    if normalize:
        den = np.sqrt(np.outer(sq, sq))
        sim = np.divide(sim, den, out=np.zeros_like(sim), where=den > 0)
    lam = min(max(float(np.float32(lam)), 0.0), 1.0)
    return scores, ids, present, sim, sq, lam, d


def _objective(scores, sim, chosen, lam):
    m = sim[:, chosen].max(axis=1) if chosen else np.zeros(len(scores))
    return lam * scores - (1.0 - lam) * m


def mmr_select(scores, ids, rows_by_pos, k, lam, normalize=False):
    """(out_scores fp32 [k], out_ids int64 [k], chosen candidate indices): the
    fp64 selection sequence; (-FLT_MAX, -1) past the present candidates."""
    scores, ids, present, sim, _, lam, _ = _setup(scores, ids, rows_by_pos, lam, normalize)
    out_s = np.full(k, -FLT_MAX, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    chosen = []
    open_ = present.copy()
    for t in range(k):
        if not open_.any():
            break
        obj = np.where(open_, _objective(scores, sim, chosen, lam), -np.inf)
        best = int(np.argmax(obj))           # the first maximum: the lowest candidate index
        chosen.append(best)
        open_[best] = False
        out_s[t], out_i[t] = np.float32(scores[best]), ids[best]
    return out_s, out_i, chosen


def tolerance(scores, ids, rows_by_pos, normalize=False):
    """2 (d + 8) 2^-24 max(1, max |score|, max |row|^2) over the present
    candidates: the bound of an fp32 dot product of length d plus a few
    roundings for the objective and the normalisation."""
    scores, _, present, _, sq, _, d = _setup(scores, ids, rows_by_pos, 0.5, normalize)
    if not present.any():
        return 2.0 * (d + 8) * 2.0 ** -24
    scale = max(1.0, float(np.abs(scores[present]).max()), float(sq[present].max()))
    return 2.0 * (d + 8) * 2.0 ** -24 * scale


def check_trace(scores, ids, rows_by_pos, k, lam, normalize, out_scores, out_ids, tol=None):
    """Replay a kernel's choices in fp64. At every step the chosen candidate
    must be present, not chosen before (by candidate index: duplicate positions
    are legal), and its fp64 objective within ``tol`` of the fp64 maximum over
    the remaining candidates; the slots past the present candidates must be
    (-FLT_MAX, -1). Returns the chosen candidate indices."""
    in_bits = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).ravel()).view(np.uint32)
    out_scores = np.ascontiguousarray(np.asarray(out_scores, dtype=np.float32).ravel())
    out_ids = np.asarray(out_ids, dtype=np.int64).ravel()
    assert out_scores.shape == (k,) and out_ids.shape == (k,)
    if tol is None:
        tol = tolerance(scores, ids, rows_by_pos, normalize)
    scores, ids, present, sim, _, lam, _ = _setup(scores, ids, rows_by_pos, lam, normalize)
    n_out = min(k, int(present.sum()))
    chosen = []
    open_ = present.copy()
    for t in range(n_out):
        match = np.flatnonzero(open_ & (ids == out_ids[t]) & (in_bits == out_scores[t:t + 1].view(np.uint32)[0]))
        assert match.size, (f"step {t}: ({out_scores[t]}, {out_ids[t]}) is no present, not yet chosen candidate "
                            f"with its original score")
        obj = np.where(open_, _objective(scores, sim, chosen, lam), -np.inf)
        # interchangeable duplicates (same position, same score): the best of them is the kernel's
        pick = int(match[np.argmax(obj[match])])
        gap = float(obj.max() - obj[pick])
        assert gap <= tol, f"step {t}: objective {obj[pick]!r} is {gap:.3e} below the maximum {obj.max()!r} (tol {tol:.3e})"
        chosen.append(pick)
        open_[pick] = False
    assert (out_ids[n_out:] == -1).all() and (out_scores[n_out:] == np.float32(-FLT_MAX)).all(), \
        f"slots past the {n_out} present candidates must be (-FLT_MAX, -1)"
    return chosen


def intra_list_diversity(ids, rows_by_pos):
    """1 - mean pairwise cosine of a list's rows (the diversity@k of the evaluation)."""
    rows = np.stack([_row(rows_by_pos, p) for p in ids])
    rows = rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-12)
    s = rows @ rows.T
    n = len(rows)
    return 1.0 - (s.sum() - np.trace(s)) / (n * (n - 1))


def clustered(seed, n, d, centres=6, noise=0.5, unit=True):
    """The tests' corpus: ``centres`` random centres, each row a centre plus
    ``noise`` N(0, I), normalised (``unit``); and one random unit query. fp64."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    rows = c[rng.integers(0, centres, size=n)] + noise * rng.standard_normal((n, d))
    if unit:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    return rows, q


def sorted_candidates(rows, q, n_cand):
    """The top ``n_cand`` rows of ``rows`` by fp64 score (stable sort: lower
    position first among equals): (scores fp32, ids int64)."""
    s = rows @ q
    order = np.argsort(-s, kind="stable")[:n_cand]
    return s[order].astype(np.float32), order.astype(np.int64)
