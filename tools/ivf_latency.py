#!/usr/bin/env python
"""Per-request latency of the IVF-Flat index against the exact Flat index.

One process, one clustered corpus of ``--rows`` x 128 (default 1,000,000;
unit-norm rows around 4,096 Gaussian centres, queries = perturbed corpus
rows), float16 and float32 storage, nq in {1, 8}, k = 100, "IVF1024,Flat",
nprobe in {1, 8, 20, 64}. The yardstick is the Flat ``OnlineSearcher`` on the
same box in the same process: its calls and the ``OnlineIVFSearcher``'s
alternate call by call (host clock around calls that end in a synchronise).

Per case: p50 / p99 of both calls and their ratio, the hipEvent time of the
coarse and the scan launches alone, the bytes the scan touches (rows of the
probed lists, averaged over the queries) and recall@k of the IVF result
against the Flat result on the same queries. The build time of each index is
reported once. ``--chunk-tiles`` adds the scan alone at other chunk floors
(rt_ivf_topk_tuning) — the measurement behind the plan's rule.

``--legs exclude`` (not in the default list): exclusion lists on the resident
IVF search, on the model of ``tools/serve_latency.py --legs exclude``. nprobe =
20, nq in {1, 8}, 166 random positions per query (MovieLens-1M's mean
history) and one case of 8,192 entries per call. Three sides alternate call by
call, 3 rounds with each side first in turn, every side ending in host arrays:
  none    the resident IVF search without exclusion;
  lists   the resident IVF search with ``exclude=`` (the scan reads the lists);
  bitmap  what a build whose scan does not read lists offers: the lists to the
          device, rt_exclusion_bitmap into a resident bitmap,
          ``search_tensors(exclude_bits=...)``, the result to the host — a path
          this change leaves as it was, run in the same process.
The bar: the p50 of ``lists`` in every round is below the MINIMUM p50 of
``bitmap`` over its rounds. ``lists`` - ``none`` is reported per round (no bar),
and the scan launch alone (hipEvent pairs) without exclusion, with lists and
with the bitmap.

``--legs mutate`` (not in the default list): HipMutableIVFFlatIndex against
HipIVFFlatIndex, both built on the same rows with the same seed (the same
centroids and assignments), nprobe = 20.
  update  ``update`` of 1, 64 and 1,024 known ids (host embeddings next to other
          corpus rows, so most change list) on the mutable index, against the only
          way a HipIVFFlatIndex reaches a state that answers with the new rows:
          ``add`` (its regroup of every row; the item is then stored twice) —
          the two alternate call by call, every call ending in a synchronise —
          and, once per storage, a full ``build``. No ratio is promised.
  search  p50 of the resident searchers of both indexes alternating call by call,
          nq in {1, 8}, 3 rounds with each side first in turn. The bar: the
          mutable side's p50 minus the other's is within 5 x the larger range of
          the two sides' p50 over the rounds.

``--legs batch`` (not in the default list): the list-major batch search
(rt_ivf_topk_batch, the ``batch_min_queries`` key) on 1M x 128 clustered rows,
nlist 1024, nprobe 20, k 100, nq in {16, 64, 256, 1024, 4096}, device-resident
queries. Three arms alternate call by call, 3 rounds with each arm first in
turn, every call ending in a synchronise:
  A  ``search_tensors`` on the per-query path (one scan block per query, probed
     list and chunk: the only path before the key existed);
  B  the same index with ``batch_min_queries = 1``;
  C  ``kernels.flatip_topk`` over the flat corpus (the exact search).
Per shape: the p50 per round and arm (with the number of calls), the hipEvent
p50 of B's scan call alone, whole and split into grouping / scan / finish
(rt_ivf_topk_batch_tuning), and one check that A and B agree bit for bit. The
bar: at nq = 4096, both storages, B's p50 in every round is below the MINIMUM
of A's p50 over its rounds; the crossover is the smallest measured nq from
which that holds for both storages. B against C is reported, not barred.

``--legs mmr`` (not in the default list): what the MMR re-rank adds to the resident
IVF search (tools/mmr_leg.py, as ``tools/serve_latency.py --legs mmr``): nprobe =
20, nq in {1, 8}, HipIVFFlatIndex and HipMutableIVFFlatIndex. Side ``plain`` is
``search(q, 100)``, side ``mmr`` the same search plus ``rt_mmr_rerank`` to k = 10 at
lambda 0.5; alternating call by call, 6 rounds with each side first in turn. p50 /
p99 per side and round, the added p50, the ratio, and the re-rank launch alone by
hipEvent pairs. No bar.

Prints one JSON line per case and a closing summary line; run it under a time
limit, e.g. ``timeout 900 python tools/ivf_latency.py > profiles/ivf_latency.txt``.
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
from rtrec_amd.serving.retrieval import HipFlatIPIndex, HipIVFFlatIndex, HipMutableIVFFlatIndex  # noqa: E402


def pct(samples_ms):
    a = np.sort(np.asarray(samples_ms, np.float64))
    return {"p50_ms": round(float(a[len(a) // 2]), 5), "p99_ms": round(float(a[min(len(a) - 1, int(len(a) * 0.99))]), 5)}


def timed_alternating(fns, calls, warmup):
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


def event_timed(fns, calls, warmup):
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
    return {name: pct([a.elapsed_time(b) for a, b in evs[name]])["p50_ms"] for name in fns}


def corpus(n, d, n_centres, n_queries, dev):
    """Clustered unit-norm rows, generated on the device (fp32), and queries on the host."""
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(n_centres, d, generator=g, device=dev), dim=1)
    which = torch.randint(0, n_centres, (n,), generator=g, device=dev)
    rows = centres[which] + 0.7 * torch.randn(n, d, generator=g, device=dev) / d ** 0.5
    rows = torch.nn.functional.normalize(rows, dim=1)
    pick = torch.randint(0, n, (n_queries,), generator=g, device=dev)
    q = torch.nn.functional.normalize(rows[pick] + 0.05 * torch.randn(n_queries, d, generator=g, device=dev), dim=1)
    return rows, q.cpu().numpy()


def recall(got, want):
    return float(np.mean([len(set(g[g >= 0]) & set(w[w >= 0])) / max(1, (w >= 0).sum()) for g, w in zip(got, want)]))


def leg_exclude(args, storage, ivf, queries, dev):
    """The exclude leg for one built index: one JSON line per (nq, entries per call)."""
    from rtrec_amd.serving.retrieval import _sorted_positions
    n, k, nprobe = ivf.current_size, args.k, args.exclude_nprobe
    ivf.nprobe = nprobe
    s = ivf.online_searcher(8)
    words = (n + 31) // 32
    rng = np.random.default_rng(3)
    cases = []
    for nq in [int(x) for x in args.nq.split(",")]:
        for per_q, what in ((166, "166_per_query"), (8192 // nq, "8192_per_call")):
            pool = [rng.choice(n, size=min(per_q, n), replace=False) for _ in range(len(queries))]
            bits = torch.zeros((nq, words), dtype=torch.int32, device=dev)
            state = {"i": 0}

            def request():
                state["i"] += 1
                o = (state["i"] * nq) % (len(queries) - nq)
                return queries[o:o + nq], pool[o:o + nq]

            def none():
                q, _ = request()
                sc, pos = s.search(q, k)
                return sc.copy(), pos.copy()

            def lists():
                q, ex = request()
                sc, pos = s.search(q, k, exclude=ex)
                return sc.copy(), pos.copy()

            def csr(ex):
                ex = [_sorted_positions(e, n) for e in ex]
                off = np.zeros(nq + 1, np.int64)
                np.cumsum([len(e) for e in ex], out=off[1:])
                return torch.from_numpy(off).to(dev), torch.from_numpy(np.concatenate(ex)).to(dev)

            def bitmap():
                q, ex = request()
                d_off, d_it = csr(ex)
                kernels.exclusion_bitmap_csr(d_off, d_it, n, out=bits)
                sc, pos = ivf.search_tensors(q, k, exclude_bits=bits)
                return sc.cpu().numpy(), pos.cpu().numpy()

            got = lists()
            state["i"] -= 1   # the same request again
            want = bitmap()
            agree = bool(np.array_equal(got[1], want[1]) and
                         np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)))
            if not agree:
                raise SystemExit(f"exclude leg {storage} nq={nq} {what}: the list side and the bitmap side differ")
            resident = (nq, k, nprobe, True) in s._graphs
            sides = {"none": none, "lists": lists, "bitmap": bitmap}
            names, rounds = list(sides), []
            for r in range(3):
                order = names[r:] + names[:r]
                res = timed_alternating({name: sides[name] for name in order}, args.calls, args.warmup)
                rounds.append({"first": order[0], **res})
            floor = min(r["bitmap"]["p50_ms"] for r in rounds)
            # the scan launch alone, on prepared device operands
            q32 = torch.nn.functional.normalize(torch.from_numpy(np.ascontiguousarray(queries[:nq])).to(dev), dim=1)
            qs = q32.to(ivf.storage_dtype)
            _, probes = kernels.flatip_topk_online(q32, ivf.centroids, nprobe)
            d_off, d_it = csr(pool[:nq])
            kernels.exclusion_bitmap_csr(d_off, d_it, n, out=bits)
            scan = lambda **kw: kernels.ivf_topk(qs, ivf.index, ivf.list_offsets, ivf.row_pos, probes,  # noqa: E731
                                                 ivf.max_list_rows, k, **kw)
            a, b = scan(exclude_lists=(d_off, d_it)), scan(exclude_bits=bits)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                raise SystemExit(f"exclude leg {storage} nq={nq} {what}: lists and bitmap differ in the scan")
            ev = event_timed({"scan_none": scan, "scan_lists": lambda: scan(exclude_lists=(d_off, d_it)),
                              "scan_bitmap": lambda: scan(exclude_bits=bits)}, min(args.calls, 300), 10)
            case = {"leg": "exclude", "storage": storage, "nq": nq, "nprobe": nprobe, "entries": what,
                    "entries_per_query": per_q, "lists_resident": resident, "sides_agree": agree, "rounds": rounds,
                    "bar": {"bitmap_min_p50_ms": floor, "lists_p50_ms": [r["lists"]["p50_ms"] for r in rounds],
                            "none_p50_ms": [r["none"]["p50_ms"] for r in rounds],
                            "lists_minus_none_p50_ms": [round(r["lists"]["p50_ms"] - r["none"]["p50_ms"], 5)
                                                        for r in rounds],
                            "lower_in_every_round": all(r["lists"]["p50_ms"] < floor for r in rounds)},
                    "scan_event_p50_ms": ev}
            print(json.dumps(case), flush=True)
            cases.append({"storage": storage, "nq": nq, "entries": what, **case["bar"]})
    return cases


def leg_filter(args, storage, rows, queries, dev):
    """Category filter on the resident IVF search path (tools/filter_leg.py: the
    sides and the checks): nprobe = --exclude-nprobe, k = --k; a request filters
    on a category that about 50 %, 10 % or 1 % of the items carry. Both host
    sides end in rt_ivf_topk's scan, so they must agree bit for bit. One JSON
    line per (nq, share)."""
    import filter_leg as fl
    n, k, nprobe = rows.shape[0], args.k, args.exclude_nprobe
    ivf = HipIVFFlatIndex({"dimension": args.dim, "metric": "cosine", "storage_dtype": storage, "nprobe": nprobe,
                           "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters,
                           "categories": [name for name, _ in fl.FILTER_SHARES]})
    ivf.build(rows, [], item_categories=fl.filter_tags(n))
    s = ivf.online_searcher(8)
    cases = []
    for nq in [int(x) for x in args.nq.split(",")]:
        for j, (name, share) in enumerate(fl.FILTER_SHARES):
            masks = (np.full(nq, 1 << j, np.uint64), np.zeros(nq, np.uint64))
            state = {"i": 0}

            def request():
                state["i"] += 1
                o = (state["i"] * nq) % (len(queries) - nq)
                return queries[o:o + nq]

            def none():
                sc, pos = s.search(request(), k)
                return sc.copy(), pos.copy()

            def tags():
                sc, pos = s.search(request(), k, tags=masks)
                return sc.copy(), pos.copy()

            def bitmap():
                sc, pos = ivf.search_tensors(request(), k, tag_filter=masks)
                return sc.cpu().numpy(), pos.cpu().numpy()

            for _ in range(max(1, (len(queries) - nq) // max(1, nq))):   # every request window
                got = tags()
                state["i"] -= 1   # the same request again
                want = bitmap()
                fl.same_scan_or_stop([torch.from_numpy(a.copy()) for a in got], [torch.from_numpy(a) for a in want],
                                     f"{storage} nq={nq} {name}")
            rounds, bar = fl.run_sides(timed_alternating, {"none": none, "tags": tags, "bitmap": bitmap},
                                       args.calls, args.warmup)
            case = {"leg": "filter", "index": "ivf", "storage": storage, "nq": nq, "nprobe": nprobe, "eligible": name,
                    "filled": float((got[1] >= 0).mean()), "rounds": rounds, "bar": bar}
            print(json.dumps(case), flush=True)
            cases.append({key: case[key] for key in ("index", "storage", "nq", "eligible", "filled", "bar")})
    return cases


def leg_mmr(args, storage, rows, queries, dev):
    """The MMR re-rank on the resident IVF search path (tools/mmr_leg.py: the sides):
    nprobe = --exclude-nprobe, side A the plain search of k = --k, side B the same
    search plus the re-rank to k = 10 at lambda 0.5; the immutable index (the inverse
    of row_pos) and the mutable one (its resident pos_slot). One JSON line per
    (index, nq)."""
    import mmr_leg
    cases = []
    for name, cls in (("ivf", HipIVFFlatIndex), ("ivf_mutable", HipMutableIVFFlatIndex)):
        ivf = cls({"dimension": args.dim, "metric": "cosine", "storage_dtype": storage, "nprobe": args.exclude_nprobe,
                   "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters})
        ivf.build(rows, [])
        s = ivf.online_searcher(8)
        for nq in [int(x) for x in args.nq.split(",")]:
            case = {"leg": "mmr", "index": name, "storage": storage, "nq": nq, "nprobe": args.exclude_nprobe,
                    **mmr_leg.measure(s, queries, nq, args.k, 10, 0.5, timed_alternating, args.calls, args.warmup)}
            print(json.dumps(case), flush=True)
            cases.append({key: case[key] for key in ("index", "storage", "nq", "added_p50_us", "mmr_over_plain_p50",
                                                     "rerank_event_ms")})
        del s, ivf
        torch.cuda.empty_cache()
    return cases


def leg_mutate(args, storage, rows, queries, dev):
    """The mutate leg for one storage dtype: one JSON line per update size and per nq."""
    n, d, k = rows.shape[0], rows.shape[1], args.k
    cfg = {"dimension": d, "metric": "cosine", "storage_dtype": storage, "nprobe": 20,
           "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters}
    ids = [f"i{p}" for p in range(n)]
    built = {}
    for name, cls in (("ivf", HipIVFFlatIndex), ("mutable", HipMutableIVFFlatIndex)):
        idx = cls(dict(cfg))
        t0 = time.perf_counter()
        idx.build(rows, ids)
        torch.cuda.synchronize()
        built[name] = (idx, round(time.perf_counter() - t0, 3))
    (ivf, t_ivf), (mut, t_mut) = built["ivf"], built["mutable"]
    caps = torch.diff(mut.list_offsets)
    print(json.dumps({"leg": "mutate", "part": "build", "storage": storage, "ivf_build_s": t_ivf,
                      "mutable_build_s": t_mut, "rows": n, "capacity": mut.capacity,
                      "max_list_rows": {"ivf": ivf.max_list_rows, "mutable": mut.max_list_rows},
                      "same_centroids": bool(torch.equal(ivf.centroids, mut.centroids)),
                      "min_capacity": int(caps.min())}), flush=True)
    out = []
    rng = np.random.default_rng(5)
    host_rows = None
    for m in [int(x) for x in args.mutate_sizes.split(",")]:
        calls = max(3, min(args.mutate_calls, 20000 // m))
        t_upd, t_add, moved = [], [], 0
        gen = mut._generation
        for c in range(calls + 2):
            pos = rng.choice(n, size=m, replace=False)
            src = torch.from_numpy(rng.integers(0, n, m)).to(dev)
            host_rows = (rows[src] + 0.02 * torch.randn(m, d, device=dev)).cpu().numpy()
            upd_ids = [ids[p] for p in pos]
            before = mut.assign[torch.from_numpy(pos).to(dev)].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mut.update(host_rows, upd_ids)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ivf.add(host_rows, upd_ids)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if c >= 2:   # two warm-up rounds
                t_upd.append((t1 - t0) * 1e3)
                t_add.append((t2 - t1) * 1e3)
                moved += int((mut.assign[torch.from_numpy(pos).to(dev)] != before).sum())
        case = {"leg": "mutate", "part": "update", "storage": storage, "m": m, "calls": calls,
                "update_in_place": pct(t_upd), "add_regroup": pct(t_add),
                "regroup_over_update_p50": round(pct(t_add)["p50_ms"] / pct(t_upd)["p50_ms"], 1),
                "rows_that_changed_list": moved, "of": calls * m,
                "regrouped_on_overflow": mut._generation != gen, "full_build_s": t_ivf}
        print(json.dumps(case), flush=True)
        out.append(case)
    # search: the mutable index (after the updates above) against a HipIVFFlatIndex on ITS rows
    del ivf
    torch.cuda.empty_cache()
    same = HipIVFFlatIndex(dict(cfg))
    same.centroids = mut.centroids
    live = torch.from_numpy(mut.vectors()).to(dev).to(mut.storage_dtype)
    same._regroup(live, None, mut.assign[: mut.current_size].clone())
    same._generation += 1
    s_mut, s_same = mut.online_searcher(8), same.online_searcher(8)
    for nq in [int(x) for x in args.nq.split(",")]:
        batches = [queries[i * nq:(i + 1) * nq] for i in range(len(queries) // nq)]
        agree = all(np.array_equal(s_mut.search(b, k)[1].copy(), s_same.search(b, k)[1].copy()) and
                    np.array_equal(s_mut.search(b, k)[0].copy(), s_same.search(b, k)[0].copy()) for b in batches)
        state = {"i": 0}

        def call(srch):
            def f():
                state["i"] += 1
                srch.search(batches[state["i"] % len(batches)], k)
            return f
        sides = {"ivf": call(s_same), "mutable": call(s_mut)}
        rounds = []
        for r in range(3):
            order = list(sides)[r % 2:] + list(sides)[:r % 2]
            res = timed_alternating({name: sides[name] for name in order}, args.calls, args.warmup)
            rounds.append({"first": order[0], **res})
        p50 = {name: [r[name]["p50_ms"] for r in rounds] for name in sides}
        rng_ = {name: round(max(v) - min(v), 5) for name, v in p50.items()}
        diff = round(float(np.median(p50["mutable"]) - np.median(p50["ivf"])), 5)
        case = {"leg": "mutate", "part": "search", "storage": storage, "nq": nq, "nprobe": 20, "results_agree": agree,
                "rounds": rounds, "p50_ms": p50, "range_ms": rng_, "mutable_minus_ivf_p50_ms": diff,
                "bar_ms": round(5 * max(rng_.values()), 5), "within_bar": diff <= 5 * max(rng_.values()),
                "plan": {"ivf": kernels.ivf_topk_plan(nq, 20, same.max_list_rows),
                         "mutable": kernels.ivf_topk_plan(nq, 20, mut.max_list_rows)}}
        print(json.dumps(case), flush=True)
        out.append(case)
    return out


def leg_batch(args, storage, rows, queries, dev):
    """The batch leg for one storage dtype: one JSON line per nq. ``queries``: fp32, on the device."""
    n, d, k, nprobe = rows.shape[0], rows.shape[1], args.k, args.batch_nprobe
    ivf = HipIVFFlatIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage, "nprobe": nprobe,
                           "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters})
    ivf.build(rows, [])
    flat = HipFlatIPIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage})
    flat.build(rows, [])
    torch.cuda.synchronize()
    lens = torch.diff(ivf.list_offsets)
    out = []
    for nq in [int(x) for x in args.batch_nq.split(",")]:
        q = queries[:nq].contiguous()
        qs = ivf._prepare(q).to(ivf.storage_dtype)
        calls = max(3, min(args.batch_calls, 20480 // nq))

        def per_query():
            ivf.batch_min_queries = None
            r = ivf.search_tensors(q, k)
            torch.cuda.synchronize()
            return r

        def batch():
            ivf.batch_min_queries = 1
            r = ivf.search_tensors(q, k)
            torch.cuda.synchronize()
            return r

        def flat_scan():
            r = kernels.flatip_topk(qs, flat.index[: flat.current_size], k)
            torch.cuda.synchronize()
            return r

        a, b, c = per_query(), batch(), flat_scan()
        agree = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
        if not agree:
            raise SystemExit(f"batch leg {storage} nq={nq}: the per-query path and the batch path differ")
        sides = {"A_per_query": per_query, "B_batch": batch, "C_flat": flat_scan}
        names, rounds = list(sides), []
        for r in range(3):
            order = names[r:] + names[:r]
            res = timed_alternating({name: sides[name] for name in order}, calls, 2)
            rounds.append({"first": order[0], **res})
        floor = min(r["A_per_query"]["p50_ms"] for r in rounds)
        # B's launches alone, on prepared device operands: a whole call fills the workspace, then each
        # stage is issued alone over it
        _, probes = kernels.flatip_topk(ivf._prepare(q), ivf.centroids, nprobe)
        ws = torch.empty(kernels.native.lib().rt_ivf_topk_batch_workspace_bytes(nq, nprobe, ivf.nlist,
                                                                                ivf.max_list_rows, k),
                         dtype=torch.uint8, device=dev)
        res = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
        scan = lambda: kernels.ivf_topk_batch(qs, ivf.index, ivf.list_offsets, ivf.row_pos, probes,  # noqa: E731
                                              ivf.max_list_rows, k, out=res, workspace_buf=ws)
        scan()
        ev = {"whole": event_timed({"s": scan}, calls, 2)["s"]}
        try:
            for name, stages in (("grouping", 1), ("scan", 2), ("finish", 4)):
                kernels.ivf_topk_batch_tuning(stages)
                ev[name] = event_timed({"s": scan}, calls, 2)["s"]
        finally:
            kernels.ivf_topk_batch_tuning(0)
        ev["coarse"] = event_timed({"s": lambda: kernels.flatip_topk(ivf._prepare(q), ivf.centroids, nprobe)}, calls,
                                   2)["s"]
        esz = 2 if storage == "float16" else 4
        case = {"leg": "batch", "storage": storage, "nq": nq, "nprobe": nprobe, "k": k, "calls_per_round": calls,
                "A_equals_B_bit_for_bit": agree, "rounds": rounds,
                "bar": {"A_min_p50_ms": floor, "B_p50_ms": [r["B_batch"]["p50_ms"] for r in rounds],
                        "A_p50_ms": [r["A_per_query"]["p50_ms"] for r in rounds],
                        "C_p50_ms": [r["C_flat"]["p50_ms"] for r in rounds],
                        "B_below_A_min_in_every_round": all(r["B_batch"]["p50_ms"] < floor for r in rounds)},
                "B_event_p50_ms": ev,
                "plan": dict(zip(("qt", "rows_per_chunk", "chunks", "items_bound", "blocks"),
                                 kernels.ivf_topk_batch_plan(nq, nprobe, ivf.nlist, ivf.max_list_rows, k))),
                "per_query_plan": kernels.ivf_topk_plan(min(nq, 32768), nprobe, ivf.max_list_rows),
                "workspace_bytes": int(ws.numel()), "max_list_rows": ivf.max_list_rows,
                "probed_row_bytes": int(lens[probes].sum().item()) * d * esz,
                f"recall_at_{k}_vs_flat": round(recall(b[1].cpu().numpy(), c[1].cpu().numpy()), 4)}
        print(json.dumps(case), flush=True)
        out.append({"storage": storage, "nq": nq, **case["bar"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--storage", default="float16,float32")
    ap.add_argument("--nprobe", default="1,8,20,64")
    ap.add_argument("--nq", default="1,8")
    ap.add_argument("--chunk-tiles", default="", help="comma list of chunk floors (256-row tiles) for the scan alone")
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--legs", default="search", help="comma list of: search (the default), exclude, mutate, batch, filter, mmr")
    ap.add_argument("--mutate-sizes", default="1,64,1024", help="known rows per update call of the mutate leg")
    ap.add_argument("--mutate-calls", type=int, default=12, help="timed update calls per size (fewer for large sizes)")
    ap.add_argument("--exclude-nprobe", type=int, default=20)
    ap.add_argument("--batch-nq", default="16,64,256,1024,4096", help="batch sizes of the batch leg")
    ap.add_argument("--batch-nprobe", type=int, default=20)
    ap.add_argument("--batch-calls", type=int, default=30,
                    help="timed calls per arm and round of the batch leg (fewer for large batches: 20,480 / nq)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = args.rows, args.dim, args.k
    rows, queries = corpus(n, d, 4096, 64, dev)
    ids = []   # positions only: the id maps are not what is measured
    summary = {"rows": n, "dim": d, "k": k, "nlist": args.nlist, "cases": []}
    legs = args.legs.split(",")
    if set(legs) - {"search", "exclude", "mutate", "batch", "filter", "mmr"}:
        raise SystemExit(f"unknown leg in {args.legs!r}")
    if "batch" in legs:
        # the same rows (the generator draws them first) and as many queries as the largest batch
        nq_max = max(int(x) for x in args.batch_nq.split(","))
        batch_queries = torch.from_numpy(corpus(n, d, 4096, nq_max, dev)[1]).to(dev)
    for storage in args.storage.split(","):
        if "batch" in legs:
            summary.setdefault("batch", []).extend(leg_batch(args, storage, rows, batch_queries, dev))
            torch.cuda.empty_cache()
            if legs == ["batch"]:
                continue
        if "mmr" in legs:
            summary.setdefault("mmr", []).extend(leg_mmr(args, storage, rows, queries, dev))
            torch.cuda.empty_cache()
            if legs == ["mmr"]:
                continue
        if "filter" in legs:
            summary.setdefault("filter", []).extend(leg_filter(args, storage, rows, queries, dev))
            torch.cuda.empty_cache()
            if legs == ["filter"]:
                continue
        if "mutate" in legs:
            summary.setdefault("mutate", []).extend(
                {key: v for key, v in case.items() if key != "rounds"} for case in leg_mutate(args, storage, rows,
                                                                                              queries, dev))
            torch.cuda.empty_cache()
            if legs == ["mutate"]:
                continue
        if "search" not in legs:
            ivf = HipIVFFlatIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage, "nprobe": 20,
                                   "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters})
            ivf.build(rows, ids)
            summary.setdefault("exclude", []).extend(leg_exclude(args, storage, ivf, queries, dev))
            del ivf
            torch.cuda.empty_cache()
            continue
        flat = HipFlatIPIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage})
        t0 = time.perf_counter()
        flat.build(rows, ids)
        torch.cuda.synchronize()
        t_flat = time.perf_counter() - t0
        ivf = HipIVFFlatIndex({"dimension": d, "metric": "cosine", "storage_dtype": storage, "nprobe": 20,
                               "index_factory": f"IVF{args.nlist},Flat", "train_iters": args.train_iters})
        t0 = time.perf_counter()
        ivf.build(rows, ids)
        torch.cuda.synchronize()
        t_ivf = time.perf_counter() - t0
        lens = torch.diff(ivf.list_offsets).cpu().numpy()
        print(json.dumps({"leg": "build", "storage": storage, "flat_build_s": round(t_flat, 3),
                          "ivf_build_s": round(t_ivf, 3), "max_list_rows": int(lens.max()),
                          "min_list_rows": int(lens.min()), "empty_lists": int((lens == 0).sum())}), flush=True)
        s_flat, s_ivf = flat.online_searcher(8), ivf.online_searcher(8)
        esz = 2 if storage == "float16" else 4
        for nq in [int(x) for x in args.nq.split(",")]:
            batches = [queries[i * nq:(i + 1) * nq] for i in range(len(queries) // nq)]
            want = np.concatenate([s_flat.search(b, k)[1].copy() for b in batches])
            for nprobe in [int(x) for x in args.nprobe.split(",")]:
                ivf.nprobe = nprobe
                got = np.concatenate([s_ivf.search(b, k)[1].copy() for b in batches])
                state = {"i": 0}

                def call(s):
                    def f():
                        state["i"] += 1
                        s.search(batches[state["i"] % len(batches)], k)
                    return f
                host = timed_alternating({"flat": call(s_flat), "ivf": call(s_ivf)}, args.calls, args.warmup)
                # the launches alone
                q32 = torch.from_numpy(np.ascontiguousarray(batches[0])).to(dev)
                qs = q32.to(ivf.storage_dtype)
                _, probes = kernels.flatip_topk_online(q32, ivf.centroids, nprobe)
                probed_rows = float(lens[probes.cpu().numpy()].sum(axis=1).mean())
                launches = {
                    "flat_online": lambda: kernels.flatip_topk_online(qs, flat.index[: flat.current_size], k),
                    "ivf_coarse": lambda: kernels.flatip_topk_online(q32, ivf.centroids, nprobe),
                    "ivf_scan": lambda: kernels.ivf_topk(qs, ivf.index, ivf.list_offsets, ivf.row_pos, probes,
                                                         ivf.max_list_rows, k),
                }
                ev = event_timed(launches, args.calls, args.warmup)
                case = {"leg": "search", "storage": storage, "nq": nq, "nprobe": nprobe,
                        "flat": host["flat"], "ivf": host["ivf"],
                        "ivf_over_flat_p50": round(host["ivf"]["p50_ms"] / host["flat"]["p50_ms"], 3),
                        "event_p50_ms": ev, "plan": kernels.ivf_topk_plan(nq, nprobe, ivf.max_list_rows),
                        "scan_bytes_per_query": int(probed_rows * d * esz),
                        "flat_bytes": int(n * d * esz),
                        f"recall_at_{k}": round(recall(got, want), 4)}
                if args.chunk_tiles:
                    sweep = {}
                    for tiles in [int(x) for x in args.chunk_tiles.split(",")]:
                        kernels.ivf_topk_tuning(tiles)
                        sweep[str(tiles)] = event_timed({"s": launches["ivf_scan"]}, args.calls, args.warmup)["s"]
                    kernels.ivf_topk_tuning(0)
                    case["scan_event_p50_ms_by_chunk_tiles"] = sweep
                print(json.dumps(case), flush=True)
                summary["cases"].append({key: case[key] for key in ("storage", "nq", "nprobe", "ivf_over_flat_p50",
                                                                     f"recall_at_{k}")})
        if "exclude" in legs:
            summary.setdefault("exclude", []).extend(leg_exclude(args, storage, ivf, queries, dev))
        del s_flat, s_ivf, flat, ivf
        torch.cuda.empty_cache()
    if "batch" in summary:
        # the crossover: the smallest measured nq from which B is below A's minimum in every round, all storages
        holds = {}
        for case in summary["batch"]:
            holds[case["nq"]] = holds.get(case["nq"], True) and case["B_below_A_min_in_every_round"]
        crossover = None
        for nq in sorted(holds, reverse=True):
            if not holds[nq]:
                break
            crossover = nq
        summary["batch_bar"] = {"holds_by_nq": {str(nq): holds[nq] for nq in sorted(holds)},
                                "met_at_largest_nq": bool(holds and holds[max(holds)]), "crossover_nq": crossover}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
