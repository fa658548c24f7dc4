"""The ``mmr`` leg shared by tools/serve_latency.py (Flat) and tools/ivf_latency.py
(IVF): what the MMR re-rank adds to a resident search call.

Two sides over ONE resident searcher, alternating call by call, every call ending
in the searcher's synchronise and a copy of its host result:
  plain  ``search(q, k_search)`` — the unchanged path: the chain and the graph key
         of a build without the re-rank;
  mmr    ``search(q, k_search, mmr=(k_out, lam))`` — the same chain plus
         ``rt_mmr_rerank`` and a smaller download.
Three rounds with ``plain`` first in a pair and three with ``mmr`` first. Reported
per round: p50 / p99 of both sides; over the rounds: the added p50 in microseconds
and the mmr / plain ratio of the p50s; and the hipEvent time of the re-rank launch
alone (the candidates of the last call still in the device buffers). No bar: the
numbers are reported as measured.
"""
import numpy as np
import torch


def measure(searcher, queries, nq, k_search, k_out, lam, timed_alternating, calls, warmup):
    state = {"i": 0}

    def request():
        state["i"] += 1
        o = (state["i"] * nq) % (len(queries) - nq)
        return queries[o:o + nq]

    def plain():
        sc, pos = searcher.search(request(), k_search)
        return sc.copy(), pos.copy()

    def mmr():
        sc, pos = searcher.search(request(), k_search, mmr=(k_out, lam))
        return sc.copy(), pos.copy()

    # lambda = 1 chooses the candidates in their order: the re-ranked call must return the plain top k_out
    a = plain()
    state["i"] -= 1
    sc, pos = searcher.search(request(), k_search, mmr=(k_out, 1.0))
    if not (np.array_equal(pos, a[1][:, :k_out]) and np.array_equal(sc, a[0][:, :k_out])):
        raise SystemExit(f"mmr leg nq={nq}: lambda = 1 does not return the plain top {k_out}")
    state["i"] -= 1   # the same request again
    got = mmr()
    sides = {"plain": plain, "mmr": mmr}
    rounds = []
    for r in range(6):
        order = list(sides) if r % 2 == 0 else list(sides)[::-1]
        rounds.append({"first": order[0], **timed_alternating({nm: sides[nm] for nm in order}, calls, warmup)})
    # the launch alone
    with searcher.lock:
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for _ in range(warmup):
            searcher._device_mmr(nq, k_search, k_out)
        torch.cuda.synchronize()
        for e0, e1 in evs:
            e0.record()
            searcher._device_mmr(nq, k_search, k_out)
            e1.record()
        torch.cuda.synchronize()
    ev = np.sort([e0.elapsed_time(e1) for e0, e1 in evs])
    added = [round((r["mmr"]["p50_ms"] - r["plain"]["p50_ms"]) * 1e3, 2) for r in rounds]
    ratio = [round(r["mmr"]["p50_ms"] / r["plain"]["p50_ms"], 4) for r in rounds]
    return {"k_search": k_search, "k_out": k_out, "lambda": lam, "rounds": rounds,
            "added_p50_us": added, "mmr_over_plain_p50": ratio,
            "rerank_event_ms": {"p50": round(float(ev[len(ev) // 2]), 5),
                                "p99": round(float(ev[min(len(ev) - 1, int(len(ev) * 0.99))]), 5)},
            "reordered": float(np.mean(np.any(got[1] != a[1][:, :k_out], axis=1)))}
