#!/usr/bin/env python
"""Per-request search latency of the serving path (not a throughput bench).

Prints ONE JSON line: p50 / p99 in milliseconds over ``--calls`` timed calls
after ``--warmup`` untimed ones, host clock (time.perf_counter) around calls
that end in a synchronise.

Legs
  serve_q1_ref  N = 1,000, d = 128, k = 50, cosine fp32, one numpy query through
                ``RetrievalEngine.retrieve(use_cache=False)`` — the shape of the
                reference's published serving number (Faiss-CPU, 0.016 ms,
                results/EVALUATION_REPORT.md:142-147).
  corpus_1m     N = 1,000,000, d = 128, k = 100, float16 and float32 storage,
                nq in {1, 8}: ``HipFlatIPIndex.search``, plus the event-timed
                top-K kernels alone (``kernel``: rt_flatip_topk; ``kernel_online``:
                the rt_flatip_topk_online pair).

Every leg is timed with ``online_max_batch`` off and on, alternating call by
call in one process (two indexes over the same rows, so neither finds its
corpus in the Infinity Cache). The ``on`` side of serve_q1_ref is also broken
down into host copy / graph replay / synchronise.

``--baseline`` uses only the API of the commit before the online path (no
``online_max_batch``, no rt_flatip_topk_online), so the same tool measures an
older build of the library: RTREC_HIP_LIB=<its librtrec_hip.so>.

Run it under a time limit, e.g. ``timeout 600 python tools/serve_latency.py``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-recommendation-system-with-feature-store_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from rtrec_amd import kernels  # noqa: E402
from rtrec_amd.serving.retrieval import HipFlatIPIndex, RetrievalEngine  # noqa: E402


def pct(samples_ms):
    a = np.sort(np.asarray(samples_ms, np.float64))
    return {"p50_ms": round(float(a[len(a) // 2]), 5), "p99_ms": round(float(a[min(len(a) - 1, int(len(a) * 0.99))]), 5),
            "min_ms": round(float(a[0]), 5), "n": int(len(a))}


def timed_alternating(fns, calls, warmup):
    """fns: {name: callable}; the callables run in turn, one call each per round."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    out = {name: [] for name in fns}
    for _ in range(calls):
        for name, f in fns.items():
            t0 = time.perf_counter()
            f()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return {name: pct(v) for name, v in out.items()}


def event_timed_alternating(fns, calls, warmup):
    """Device time of each callable's launches (hipEvent pairs), alternating."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    evs = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
           for name in fns}
    for i in range(calls):
        for name, f in fns.items():
            a, b = evs[name][i]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return {name: pct([a.elapsed_time(b) for a, b in evs[name]]) for name in fns}


def leg_serve_q1_ref(args):
    n, d, k = 1000, 128, 50
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = [f"item_{i}" for i in range(n)]
    qs = rng.standard_normal((64, d)).astype(np.float32)
    base = {"index_type": "hip_flat", "embedding_dim": d, "top_k": k}
    engines = {"off": RetrievalEngine(dict(base))}
    if args.baseline:  # two engines in both modes: the same alternation between two corpora
        engines["off2"] = RetrievalEngine(dict(base))
    else:
        engines["on"] = RetrievalEngine(dict(base, hip_flat={"online_max_batch": 8}))
    for e in engines.values():
        e.build_index(x, ids)
    state = {"i": 0}

    def call(e):
        def f():
            state["i"] += 1
            e.retrieve(qs[state["i"] % 64], k=k, use_cache=False)
        return f
    res = timed_alternating({name: call(e) for name, e in engines.items()}, args.calls, args.warmup)
    res["reference_faiss_cpu_ms"] = 0.016
    if not args.baseline:
        # the on side in pieces: host copy -> graph replay (launch) -> synchronise
        s = engines["on"].index._online
        g = s._graphs[(1, k)]
        stream = torch.cuda.current_stream()
        parts = {"host_copy": [], "graph_replay": [], "synchronise": [], "lists": []}
        idx = engines["on"].index
        from rtrec_amd.serving.retrieval import _lists_from_positions
        for i in range(args.calls):
            q = torch.as_tensor(qs[i % 64]).reshape(1, -1)
            t0 = time.perf_counter()
            s._h_q[:1].copy_(q)
            t1 = time.perf_counter()
            g.replay()
            t2 = time.perf_counter()
            stream.synchronize()
            t3 = time.perf_counter()
            _lists_from_positions(s._h_s_np[:k].reshape(1, k), s._h_p_np[:k].reshape(1, k), idx.id_map, k, None)
            t4 = time.perf_counter()
            for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[name].append(dt * 1e3)
        res["on_breakdown"] = {name: pct(v) for name, v in parts.items()}
    return res


def leg_corpus_1m(args):
    n, d, k = args.rows, 128, 100
    out = {}
    ids = [str(i) for i in range(n)]
    for storage in ("float16", "float32"):
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((n, d), generator=g, device="cuda")
        cfg = {"dimension": d, "metric": "cosine", "storage_dtype": storage}
        idxs = {"off": HipFlatIPIndex(dict(cfg))}
        idxs["on" if not args.baseline else "off2"] = HipFlatIPIndex(
            dict(cfg) if args.baseline else dict(cfg, online_max_batch=8))
        for ix in idxs.values():  # two copies of the rows in both modes: the same cache pressure
            ix.build(x, ids)
        del x
        qs = np.random.default_rng(2).standard_normal((64, d)).astype(np.float32)
        for nq in (1, 8):
            state = {"i": 0}

            def call(ix):
                def f():
                    state["i"] += 1
                    o = (state["i"] * nq) % (64 - nq)
                    ix.search(qs[o:o + nq], k)
                return f
            res = timed_alternating({name: call(ix) for name, ix in idxs.items()}, args.calls, args.warmup)
            # the kernels alone, on prepared device queries
            kq = {}
            for name, ix in idxs.items():
                q = torch.nn.functional.normalize(torch.from_numpy(qs[:nq]).cuda(), dim=1).to(ix.storage_dtype)
                rows = ix.index[: ix.current_size]
                if name == "on":
                    kq["kernel_online"] = (lambda q=q, rows=rows: kernels.flatip_topk_online(q, rows, k))
                else:
                    kq["kernel" if name == "off" else "kernel2"] = (lambda q=q, rows=rows: kernels.flatip_topk(q, rows, k))
            res.update(event_timed_alternating(kq, min(args.calls, 300), 10))
            bytes_ = n * d * (2 if storage == "float16" else 4)
            res["corpus_bytes"] = bytes_
            res["pass_at_8TBps_ms"] = round(bytes_ / 8e12 * 1e3, 5)
            out[f"{storage}_nq{nq}"] = res
        del idxs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline", action="store_true", help="only the API of the commit before the online path")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the corpus_1m leg")
    ap.add_argument("--legs", default="serve_q1_ref,corpus_1m")
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be positive")
    torch.cuda.init()
    res = {"tool": "serve_latency", "baseline": bool(args.baseline), "calls": args.calls, "warmup": args.warmup,
           "lib": os.environ.get("RTREC_HIP_LIB", "in-tree"), "device": torch.cuda.get_device_name(0)}
    legs = {"serve_q1_ref": leg_serve_q1_ref, "corpus_1m": leg_corpus_1m}
    for name in args.legs.split(","):
        if name not in legs:
            ap.error(f"unknown leg {name!r}")
        res[name] = legs[name](args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
