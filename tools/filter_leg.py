"""What the ``filter`` legs of tools/serve_latency.py and tools/ivf_latency.py share:
the tags, the three sides and what a disagreement between them means.

Sides, alternating call by call, 3 rounds with each side first in turn, every
side ending in host arrays:
  none    the resident searcher without a filter;
  tags    the resident searcher with ``tags=`` (the scan tests the tags);
  bitmap  the route without a native filter: rt_tag_filter_bitmap, then
          ``search_tensors(exclude_bits=...)`` and the result to the host.

Checks before anything is timed. ``same_scan`` (the caller's closure: the scan
with its own filter against the SAME scan reading the filter's bitmap) must
agree bit for bit, or the leg stops. The two host sides may go through
different kernels (Flat: the batch kernel behind ``search_tensors``, whose
16-bit scores round differently from the online chain's in the last bit), so
ids may swap between near ties: every differing slot must hold a score that is the
slot's score on the other side within ``TIE_RTOL``; anything else stops the leg."""
import numpy as np
import torch

FILTER_SHARES = (("50pct", 0.5), ("10pct", 0.1), ("1pct", 0.01))


def filter_tags(n, seed=7):
    """uint64 [n]: bit j set with the probability of FILTER_SHARES[j], independently."""
    rng = np.random.default_rng(seed)
    tags = np.zeros(n, np.uint64)
    for j, (_, share) in enumerate(FILTER_SHARES):
        tags |= (rng.random(n) < share).astype(np.uint64) << np.uint64(j)
    return tags


# Unit-norm rows and queries, d = 128: a score is a sum of 128 exact products whose absolute
# values sum to at most 1; two fp32 accumulation orders differ by at most about d x 2^-24 of
# that, 7.6e-6, against top scores of 0.25 and more: 2^-15 relative covers it.
TIE_RTOL = 2.0 ** -15


def compare_sides(got, want, tie_rtol=TIE_RTOL):
    """got / want: (scores [nq, k], ids [nq, k]). Returns the agreement record;
    raises SystemExit for a difference that is no near-tie swap."""
    gs, gi = got
    ws, wi = want
    rec = {"ids": bool(np.array_equal(gi, wi)),
           "scores": bool(np.array_equal(gs.view(np.uint32), ws.view(np.uint32))),
           "differing_slots": int((gi != wi).sum()), "max_rel_score_gap": 0.0}
    for q in range(gi.shape[0]):
        for j in np.nonzero(gi[q] != wi[q])[0]:
            # the slot's two scores are those of two different rows: a swap or a k-th boundary
            gap = abs(float(gs[q, j]) - float(ws[q, j])) / max(abs(float(ws[q, j])), 1e-30)
            rec["max_rel_score_gap"] = max(rec["max_rel_score_gap"], gap)
            if gap > tie_rtol:
                raise SystemExit(f"filter leg: query {q} slot {j}: ids {gi[q, j]} vs {wi[q, j]} with scores "
                                 f"{gs[q, j]} vs {ws[q, j]}: no near tie")
    return rec


def run_sides(timed_alternating, sides, calls, warmup):
    names, rounds = list(sides), []
    for r in range(3):
        order = names[r:] + names[:r]
        rounds.append({"first": order[0], **timed_alternating({nm: sides[nm] for nm in order}, calls, warmup)})
    bar = {side: [r[side]["p50_ms"] for r in rounds] for side in names}
    bar["tags_below_bitmap_min_in_every_round"] = max(bar["tags"]) < min(bar["bitmap"])
    return rounds, bar


def same_scan_or_stop(a, b, what):
    if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
        raise SystemExit(f"filter leg {what}: the scan's filter and the same scan over the filter's bitmap differ")
