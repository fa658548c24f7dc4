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

  embed_b1      one user row to its embedding on the host: ``get_user_embeddings(
                ...).cpu().numpy()`` (``two_step``) against ``OnlineRecommender.embed``
                (``recommender``); the reference publishes 0.059 ms.
  serve_e2e     one user row to its lists at N = 1,000, d = 128, k = 50, cosine fp32:
                ``get_user_embeddings`` -> ``.cpu().numpy()`` -> ``RetrievalEngine.
                retrieve(use_cache=False)`` with ``online_max_batch = 8`` against
                ``OnlineRecommender.recommend``; the reference publishes 0.101 ms.
                Both legs run with the service-default tower (input 10) and with
                the C2 user tower by id (``user_ids`` into a resident table), 3
                rounds each way; ``bar``: the recommender's p50 of every round
                against the two-step path's minimum p50 over its rounds.
  tower_kernel  (not in the default list) rt_tower_infer_f32 launches alone at m = 1
                and 8, for ``rocprofv3 --kernel-trace -- python tools/serve_latency.py
                --legs tower_kernel --towers service``.

  mutate        (not in the default list) N = 1,000,000, d = 128, cosine, float16 and
                float32, ``mutable: True``: ``update`` of 1 and of 64 rows, ``remove``
                of 1 and of 1,000 ids (the corpus restored between calls, outside
                the timing) against ``index.build`` on the device-resident surviving
                rows with their ids — all an index without the option offers. The
                sides alternate call by call, 3 rounds each way, ``--mutate-calls``
                calls per case and round; ``bar``: the p50 of every case in every
                round against the build's minimum p50 over its rounds. Also the
                compaction alone by hipEvent pairs ((bytes read + written) / time
                as a fraction of 8 TB/s) and the host bookkeeping of ``remove``
                (the call minus its device work).

  exclude       (not in the default list) seen-item exclusion on the resident search:
                N = --rows, d = 128, k = 100, float16 and float32, nq in {1, 8}, 166
                random positions per query. Sides ``none`` (no exclusion), ``lists``
                (``OnlineSearcher.search(exclude=...)``) and ``bitmap`` (what a build
                without the list entry offers: rt_exclusion_bitmap into a resident
                bitmap + ``search_tensors(exclude_bits=...)``) alternate call by call,
                3 rounds with each side first in turn; ``bar``: the p50 of ``lists``
                in every round against the minimum p50 of ``bitmap`` over its rounds.
                Plus the online kernel pair alone by hipEvent pairs, three ways
                (no exclusion, lists, dense bitmap). The leg stops if the list and
                bitmap forms of the online kernel differ in any bit, or if the two
                sides return different ids (``sides_agree`` also records whether their
                scores are equal; the bitmap side runs the batch kernel).

  mmr           (not in the default list) the MMR re-rank on the resident search
                (tools/mmr_leg.py): N = --rows, d = 128, float16 and float32, nq in
                {1, 8}. Side ``plain`` is ``OnlineSearcher.search(q, 100)``, side
                ``mmr`` the same search plus ``rt_mmr_rerank`` to k = 10 at lambda
                0.5 (``search(q, 100, mmr=(10, 0.5))``); they alternate call by call,
                6 rounds with each side first in turn. Reported: p50 / p99 per side
                and round, the added p50 and the ratio, and the re-rank launch alone
                by hipEvent pairs. No bar.

The first two legs are timed with ``online_max_batch`` off and on, alternating
call by call in one process (two indexes over the same rows, so neither finds
its corpus in the Infinity Cache). The ``on`` side of serve_q1_ref and the
recommender side of serve_e2e are also broken down into host copy / graph
replay / synchronise / list building.

``--baseline`` uses only the API of the commit before the online path (no
``online_max_batch``, no rt_flatip_topk_online, no OnlineRecommender: the new
legs time their two-step side alone), so the same tool measures an older build
of the library: RTREC_HIP_LIB=<its librtrec_hip.so>.

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


# (name, user-tower input width, hidden layers, served by id from a resident user table)
TOWERS = (("service", 10, [512, 256, 128], False), ("c2_by_id", 3, [256, 128], True))
N_USERS = 6040  # MovieLens-1M


def _towers(args):
    want = args.towers.split(",")
    unknown = [t for t in want if t not in [x[0] for x in TOWERS]]
    if unknown:
        raise SystemExit(f"unknown tower {unknown}")
    return [t for t in TOWERS if t[0] in want]


def _request_setup(args, in_dim, hidden, by_id):
    """Model, index and the two sides of one request at the reference's serving
    shape (N = 1,000, d = 128, k = 50, cosine fp32): the two-step path of the
    parent (get_user_embeddings -> .cpu().numpy() -> RetrievalEngine.retrieve,
    online_max_batch = 8) and OnlineRecommender."""
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    n, d, k = 1000, 128, 50
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TwoTowerModel(UserTower(in_dim, d, hidden), ItemTower(20, d, [64], use_content_embedding=False))
    model = model.to(dev).eval()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = [f"item_{i}" for i in range(n)]
    feats = rng.standard_normal((N_USERS, in_dim)).astype(np.float32)
    table = torch.from_numpy(feats).to(dev)
    base = {"index_type": "hip_flat", "embedding_dim": d, "top_k": k}
    eng = RetrievalEngine(dict(base) if args.baseline else dict(base, hip_flat={"online_max_batch": 8}))
    eng.build_index(x, ids)
    state = {"i": 0}

    def user():
        state["i"] += 1
        return (state["i"] * 7919) % N_USERS

    def two_step_embed():
        u = user()
        with torch.no_grad():
            row = table[u:u + 1] if by_id else torch.from_numpy(feats[u:u + 1]).to(dev)
            return model.get_user_embeddings({"numerical": row, "categorical": {}}).cpu().numpy()

    def two_step_e2e():
        return eng.retrieve(two_step_embed(), k=k, use_cache=False)

    sides_embed, sides_e2e, rec = {"two_step": two_step_embed}, {"two_step": two_step_e2e}, None
    if not args.baseline:
        from rtrec_amd.serving.online import OnlineRecommender
        eng2 = RetrievalEngine(dict(base))   # its own copy of the corpus, as in the other legs
        eng2.build_index(x, ids)
        rec = OnlineRecommender(model, eng2, max_batch=8, user_table=table if by_id else None)
        if by_id:
            sides_embed["recommender"] = lambda: rec.embed(user_ids=[user()])
            sides_e2e["recommender"] = lambda: rec.recommend(user_ids=[user()], k=k)
        else:
            sides_embed["recommender"] = lambda: rec.embed(feats[user()])
            sides_e2e["recommender"] = lambda: rec.recommend(feats[user()], k=k)
    return sides_embed, sides_e2e, rec, feats, k


def _rounds(sides, args):
    """3 rounds each way (the order of the two sides within a call pair swapped),
    alternating call by call; the bar: the recommender's p50 of every round is
    below the two-step path's MINIMUM p50 over its rounds."""
    out = []
    for r in range(6):
        order = list(sides) if r % 2 == 0 else list(sides)[::-1]
        res = timed_alternating({name: sides[name] for name in order}, args.calls, args.warmup)
        out.append({"first": order[0], **res})
    verdict = None
    if "recommender" in sides:
        floor = min(r["two_step"]["p50_ms"] for r in out)
        verdict = {"two_step_min_p50_ms": floor,
                   "recommender_p50_ms": [r["recommender"]["p50_ms"] for r in out],
                   "lower_in_every_round": all(r["recommender"]["p50_ms"] < floor for r in out)}
    return {"rounds": out, "bar": verdict}


def _breakdown(rec, feats, k, by_id, calls):
    """OnlineRecommender.recommend at nq = 1 in pieces."""
    from rtrec_amd.serving.retrieval import _lists_from_positions
    s = rec._searcher
    g = rec._graphs[(1, k, by_id)]
    stream = torch.cuda.current_stream()
    parts = {"host_copy": [], "graph_replay": [], "synchronise": [], "lists": []}
    for i in range(calls):
        u = (i * 7919) % N_USERS
        t0 = time.perf_counter()
        if by_id:
            rec._h_ids_np[:1] = u
        else:
            rec._h_x[:1].copy_(torch.as_tensor(feats[u]).reshape(1, -1))
        t1 = time.perf_counter()
        g.replay()
        t2 = time.perf_counter()
        stream.synchronize()
        t3 = time.perf_counter()
        _lists_from_positions(s._h_s_np[:k].reshape(1, k), s._h_p_np[:k].reshape(1, k), rec.index.id_map, k, None)
        t4 = time.perf_counter()
        for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[name].append(dt * 1e3)
    return {name: pct(v) for name, v in parts.items()}


def leg_embed_b1(args):
    out = {"reference_ms": 0.059}
    for name, in_dim, hidden, by_id in _towers(args):
        sides, _, _, _, _ = _request_setup(args, in_dim, hidden, by_id)
        out[name] = _rounds(sides, args)
    return out


def leg_serve_e2e(args):
    out = {"reference_ms": 0.101}
    for name, in_dim, hidden, by_id in _towers(args):
        _, sides, rec, feats, k = _request_setup(args, in_dim, hidden, by_id)
        out[name] = _rounds(sides, args)
        if rec is not None:
            out[name]["recommender_breakdown"] = _breakdown(rec, feats, k, by_id, args.calls)
    return out


def leg_tower_kernel(args):
    """rt_tower_infer_f32 alone, for a kernel trace: both towers, m = 1 and 8."""
    for name, in_dim, hidden, by_id in _towers(args):
        _, _, rec, feats, _ = _request_setup(args, in_dim, hidden, by_id)
        rec._d_ids.copy_(torch.arange(8, device=rec._d_ids.device))
        rec._d_x.copy_(torch.from_numpy(feats[:8]))
        for m in (1, 8):
            for _ in range(args.calls):
                rec._tower(m, by_id)
            torch.cuda.synchronize()
    return {"launches_per_tower_and_m": args.calls}


def leg_mutate(args):
    """``update`` / ``remove`` of a ``mutable`` index at N = ``--rows``, d = 128,
    cosine, against the only thing an index without the option offers:
    ``index.build`` on the device-resident surviving rows with their ids."""
    n, d = args.rows, 128
    calls = max(1, args.mutate_calls)
    out = {"calls_per_round": calls}
    ids = [str(i) for i in range(n)]
    rng = np.random.default_rng(3)
    pick = {m: rng.choice(n, m, replace=False) for m in (1, 64, 1000)}
    for storage in ("float16", "float32"):
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((n, d), generator=g, device="cuda")
        new = {m: torch.randn((2, m, d), generator=g, device="cuda") for m in (1, 64)}
        cfg = {"dimension": d, "metric": "cosine", "storage_dtype": storage}
        ix = HipFlatIPIndex(dict(cfg, mutable=True))
        ix.build(x, ids)
        # the parent's side: a build on the surviving rows of the largest removal (the
        # fewest rows any case leaves it: the cheapest build) — rows and ids made outside the timing
        gone = np.zeros(n, dtype=bool)
        gone[pick[1000]] = True
        x_surv = x[torch.from_numpy(~gone).cuda()].contiguous()
        ids_surv = [i for i, dead in zip(ids, gone.tolist()) if not dead]
        rebuilt = HipFlatIPIndex(dict(cfg))
        snap = (ix.index, ix._ids, ix.id_map, ix.reverse_id_map, ix.current_size)
        state = {"i": 0}

        def restore():
            # remove is out of place and builds new id structures: the old ones are intact
            ix.index, ix._ids, ix.id_map, ix.reverse_id_map, ix.current_size = snap
            ix._generation += 1

        def update(m):
            upd_ids = [ids[p] for p in pick[m]]

            def f():
                state["i"] += 1
                ix.update(new[m][state["i"] % 2], upd_ids)   # other values every call; nothing to restore
                torch.cuda.synchronize()
            return f

        def remove(m):
            rm_ids = [ids[p] for p in pick[m]]

            def f():
                ix.remove(rm_ids)
                torch.cuda.synchronize()
            return f

        def build():
            rebuilt.build(x_surv, ids_surv)
            torch.cuda.synchronize()

        sides = {"update_1": update(1), "update_64": update(64), "remove_1": remove(1), "remove_1000": remove(1000),
                 "build": build}
        for f in sides.values():   # warm: kernels loaded, buffers of the allocator sized
            f()
            restore()
        rounds = []
        for r in range(6):  # 3 rounds each way: the parent's build last, then first
            order = list(sides) if r % 2 == 0 else ["build"] + [s for s in sides if s != "build"]
            samples = {name: [] for name in sides}
            for _ in range(calls):
                for name in order:
                    t0 = time.perf_counter()
                    sides[name]()
                    samples[name].append((time.perf_counter() - t0) * 1e3)
                    if name.startswith("remove"):
                        restore()   # outside the timed region
            rounds.append({"first": order[0], **{name: pct(v) for name, v in samples.items()}})
        floor = min(r["build"]["p50_ms"] for r in rounds)
        bar = {"build_min_p50_ms": floor}
        for name in sides:
            if name != "build":
                p50s = [r[name]["p50_ms"] for r in rounds]
                bar[name] = {"p50_ms": p50s, "lower_in_every_round": all(p < floor for p in p50s)}
        # the compaction alone (hipEvent pairs): offsets + move launches on the index's rows
        rows = ix.index[:n]
        dst = torch.empty_like(rows)
        dev = {}
        for m in (1, 1000):
            keep = np.ones(-(-n // 32) * 32, dtype=bool)
            keep[pick[m]] = False
            bits = torch.from_numpy(np.packbits(keep, bitorder="little").view("<u4").view(np.int32).copy()).cuda()
            t = event_timed_alternating({"compact": lambda bits=bits: kernels.rows_compact(rows, bits, dst)}, 50, 5)
            moved = (2 * n - m) * rows.shape[1] * rows.element_size()   # bytes read + bytes written
            t["compact"]["bytes_moved"] = moved
            t["compact"]["fraction_of_8TBps"] = round(moved / (t["compact"]["p50_ms"] * 1e-3) / 8e12, 4)
            dev[f"remove_{m}"] = t["compact"]
        # host bookkeeping of remove = the call minus its device work (the launches come
        # last in remove, after the id structures are rebuilt, so the two add up)
        host = {name: round(min(r[name]["p50_ms"] for r in rounds) - dev[name]["p50_ms"], 5) for name in dev}
        out[storage] = {"rounds": rounds, "bar": bar, "compaction_device": dev, "remove_host_ms": host,
                        "c5_gather_yardstick_fraction_of_8TBps": [0.72, 0.77]}
        del ix, rebuilt, x, x_surv, rows, dst, snap
        torch.cuda.empty_cache()
    return out


def leg_exclude(args):
    """Seen-item exclusion on the resident search path: N = --rows, d = 128,
    k = 100, float16 and float32 rows, nq = 1 and 8, 166 random positions per
    query (MovieLens-1M's mean history). Three sides, alternating call by call,
    3 rounds with each side first in turn, every side ending in the id lists:
      none   the resident searcher without exclusion;
      lists  the resident searcher with ``exclude=`` (the scan reads the lists);
      bitmap what a build without the list entry offers: the lists to the device,
             rt_exclusion_bitmap into a resident bitmap, search_tensors(
             exclude_bits=...), the result to the host.
    The bar: the p50 of ``lists`` in every round is below the MINIMUM p50 of
    ``bitmap`` over its rounds. Then the kernel pair alone (hipEvent pairs):
    without exclusion, with lists, and with the dense bitmap through
    rt_flatip_topk_online."""
    from rtrec_amd.serving.retrieval import _lists_from_positions, _sorted_positions
    n, d, k, per_q = args.rows, 128, 100, 166
    out = {}
    ids = [str(i) for i in range(n)]
    rng = np.random.default_rng(3)
    qs = rng.standard_normal((64, d)).astype(np.float32)
    pool = [rng.choice(n, size=min(per_q, n), replace=False) for _ in range(64)]
    for storage in ("float16", "float32"):
        g = torch.Generator(device="cuda").manual_seed(1)
        ix = HipFlatIPIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage})
        ix.build(torch.randn((n, d), generator=g, device="cuda"), ids)
        s = ix.online_searcher(8)
        words = (n + 31) // 32
        for nq in (1, 8):
            bits = torch.zeros((nq, words), dtype=torch.int32, device="cuda")
            state = {"i": 0}

            def request():
                state["i"] += 1
                o = (state["i"] * nq) % (64 - nq)
                return qs[o:o + nq], pool[o:o + nq]

            def none():
                q, _ = request()
                with s.lock:
                    sc, pos = s.search(q, k)
                    return _lists_from_positions(sc, pos, ix.id_map, k, None)

            def lists():
                q, ex = request()
                with s.lock:
                    sc, pos = s.search(q, k, exclude=ex)
                    return _lists_from_positions(sc, pos, ix.id_map, k, None)

            def bitmap():
                q, ex = request()
                ex = [_sorted_positions(e, n) for e in ex]
                off = np.zeros(nq + 1, np.int64)
                np.cumsum([len(e) for e in ex], out=off[1:])
                kernels.exclusion_bitmap_csr(torch.from_numpy(off).cuda(), torch.from_numpy(np.concatenate(ex)).cuda(),
                                             n, out=bits)
                sc, pos = ix.search_tensors(q, k, exclude_bits=bits)
                return _lists_from_positions(sc.cpu().numpy(), pos.cpu().numpy(), ix.id_map, k, None)

            # the kernel pair alone, on prepared device queries and resident operands: first
            # that the list form and the bitmap form agree bit for bit, timed after the rounds
            q = torch.nn.functional.normalize(torch.from_numpy(qs[:nq]).cuda(), dim=1).to(ix.storage_dtype)
            rows = ix.index[: ix.current_size]
            ex = [_sorted_positions(e, n) for e in pool[:nq]]
            off = np.zeros(nq + 1, np.int64)
            np.cumsum([len(e) for e in ex], out=off[1:])
            d_off, d_it = torch.from_numpy(off).cuda(), torch.from_numpy(np.concatenate(ex)).cuda()
            kernels.exclusion_bitmap_csr(d_off, d_it, n, out=bits)
            a = kernels.flatip_topk_online(q, rows, k, exclude_lists=(d_off, d_it))
            b = kernels.flatip_topk_online(q, rows, k, exclude_bits=bits)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                raise SystemExit(f"exclude leg {storage} nq={nq}: lists and bitmap differ in the online kernel")
            sides = {"none": none, "lists": lists, "bitmap": bitmap}
            got = lists()
            state["i"] -= 1  # the same request again
            ref = bitmap()
            agree = {"ids": got[0] == ref[0], "scores": got[1] == ref[1]}
            if not agree["ids"]:
                raise SystemExit(f"exclude leg {storage} nq={nq}: the list side and the bitmap side return "
                                 f"different ids: {got[0][0][:5]} vs {ref[0][0][:5]}")
            names, rounds = list(sides), []
            for r in range(3):
                order = names[r:] + names[:r]
                res = timed_alternating({name: sides[name] for name in order}, args.calls, args.warmup)
                rounds.append({"first": order[0], **res})
            floor = min(r["bitmap"]["p50_ms"] for r in rounds)
            res = {"rounds": rounds, "bar": {
                "bitmap_min_p50_ms": floor, "lists_p50_ms": [r["lists"]["p50_ms"] for r in rounds],
                "none_p50_ms": [r["none"]["p50_ms"] for r in rounds],
                "lower_in_every_round": all(r["lists"]["p50_ms"] < floor for r in rounds)}}
            res["sides_agree"] = agree
            res["kernels"] = event_timed_alternating({
                "kernel_none": lambda: kernels.flatip_topk_online(q, rows, k),
                "kernel_lists": lambda: kernels.flatip_topk_online(q, rows, k, exclude_lists=(d_off, d_it)),
                "kernel_bitmap": lambda: kernels.flatip_topk_online(q, rows, k, exclude_bits=bits),
            }, min(args.calls, 300), 10)
            out[f"{storage}_nq{nq}"] = res
        del s, ix
        torch.cuda.empty_cache()
    return out


def leg_filter(args):
    """Category filter on the resident Flat search path (tools/filter_leg.py: the
    sides and the checks): N = --rows, d = 128, k = 100, float16 and float32
    rows, nq = 1 and 8; a request filters on a category that about 50 %, 10 % or
    1 % of the items carry."""
    import filter_leg as fl
    n, d, k = args.rows, 128, 100
    out = {}
    qs = np.random.default_rng(3).standard_normal((64, d)).astype(np.float32)
    tags_np = fl.filter_tags(n)
    for storage in ("float16", "float32"):
        g = torch.Generator(device="cuda").manual_seed(1)
        ix = HipFlatIPIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage,
                             "categories": [name for name, _ in fl.FILTER_SHARES]})
        ix.build(torch.randn((n, d), generator=g, device="cuda"), [], item_categories=tags_np)
        s = ix.online_searcher(8)
        rows = ix.index[: ix.current_size]
        for nq in (1, 8):
            for j, (name, share) in enumerate(fl.FILTER_SHARES):
                masks = (np.full(nq, 1 << j, np.uint64), np.zeros(nq, np.uint64))
                state = {"i": 0}

                def request():
                    state["i"] += 1
                    o = (state["i"] * nq) % (64 - nq)
                    return qs[o:o + nq]

                def none():
                    sc, pos = s.search(request(), k)
                    return sc.copy(), pos.copy()

                def tags():
                    sc, pos = s.search(request(), k, tags=masks)
                    return sc.copy(), pos.copy()

                def bitmap():
                    sc, pos = ix.search_tensors(request(), k, tag_filter=masks)
                    return sc.cpu().numpy(), pos.cpu().numpy()

                # the scan's own filter against the same scan reading the filter's bitmap: every
                # one of the 64 - nq request windows, bit for bit
                d_any, d_none = (torch.from_numpy(m.view(np.int64).copy()).cuda() for m in masks)
                bits = kernels.tag_filter_bitmap(ix._tags, d_any, d_none, nq, n_items=n)
                for o in range(0, 64 - nq, max(1, nq)):
                    dq = torch.nn.functional.normalize(torch.from_numpy(qs[o:o + nq]).cuda(), dim=1).to(ix.storage_dtype)
                    fl.same_scan_or_stop(kernels.flatip_topk_online(dq, rows, k, tag_filter=(ix._tags, d_any, d_none)),
                                         kernels.flatip_topk_online(dq, rows, k, exclude_bits=bits),
                                         f"{storage} nq={nq} {name} window {o}")
                got = tags()
                state["i"] -= 1  # the same request again
                agree = fl.compare_sides(got, bitmap())
                rounds, bar = fl.run_sides(timed_alternating, {"none": none, "tags": tags, "bitmap": bitmap},
                                           args.calls, args.warmup)
                out[f"{storage}_nq{nq}_{name}"] = {"rounds": rounds, "bar": bar, "sides_agree": agree,
                                                   "filled": float((got[1] >= 0).mean())}
        del s, ix, rows
        torch.cuda.empty_cache()
    return out


def leg_mmr(args):
    """The MMR re-rank on the resident Flat search path (tools/mmr_leg.py: the sides):
    N = --rows, d = 128, float16 and float32 rows, nq = 1 and 8; side A the plain
    search of k = 100, side B the same search plus the re-rank to k = 10, lambda 0.5."""
    import mmr_leg
    n, d = args.rows, 128
    out = {}
    qs = np.random.default_rng(3).standard_normal((64, d)).astype(np.float32)
    for storage in ("float16", "float32"):
        g = torch.Generator(device="cuda").manual_seed(1)
        ix = HipFlatIPIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage})
        ix.build(torch.randn((n, d), generator=g, device="cuda"), [])
        s = ix.online_searcher(8)
        for nq in (1, 8):
            out[f"{storage}_nq{nq}"] = mmr_leg.measure(s, qs, nq, 100, 10, 0.5, timed_alternating, args.calls,
                                                       args.warmup)
        del s, ix
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline", action="store_true", help="only the API of the commit before the online path")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the corpus_1m and mutate legs")
    ap.add_argument("--mutate-calls", type=int, default=3,
                    help="timed calls per case and round of the mutate leg (a call at 10^6 rows is O(N) host work)")
    ap.add_argument("--legs", default="serve_q1_ref,corpus_1m,embed_b1,serve_e2e")
    ap.add_argument("--towers", default=",".join(t[0] for t in TOWERS),
                    help="towers of the embed_b1 / serve_e2e / tower_kernel legs")
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be positive")
    torch.cuda.init()
    res = {"tool": "serve_latency", "baseline": bool(args.baseline), "calls": args.calls, "warmup": args.warmup,
           "lib": os.environ.get("RTREC_HIP_LIB", "in-tree"), "device": torch.cuda.get_device_name(0)}
    legs = {"serve_q1_ref": leg_serve_q1_ref, "corpus_1m": leg_corpus_1m, "embed_b1": leg_embed_b1,
            "serve_e2e": leg_serve_e2e, "tower_kernel": leg_tower_kernel, "mutate": leg_mutate,
            "exclude": leg_exclude, "filter": leg_filter, "mmr": leg_mmr}
    for name in args.legs.split(","):
        if name not in legs:
            ap.error(f"unknown leg {name!r}")
        res[name] = legs[name](args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
