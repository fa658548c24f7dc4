#!/usr/bin/env python3
"""A/B of the list-metrics kernels against the plain torch composition on the
same device (not a test).

Arms, diversity and novelty together at k = 10 and 100:
  kernel   rtrec_amd.evaluation.list_metrics_tensors (rt_list_metrics +
           rt_list_metrics_reduce, fp64)
  torch    index_select -> normalise -> bmm -> upper-triangle mean per k, and an
           index_select of the self-information table (fp32 arithmetic)

Shapes: 6,040 lists x 100 over a 3,900 x 64 fp32 table (the ML-1M evaluation),
and 65,536 lists x 100 over a 1,000,000 x 128 fp16 table. Every arm is warmed,
then timed in windows of at least --window seconds that end in a device
synchronise; the arms alternate inside every round. Rule (the project's A/B
rule): the kernel arm counts as faster when it is below the torch arm in every
round and the mean difference exceeds five times the larger arm's range.

Byte model of the gather: n_rows * list_len * d * sizeof(elem) bytes (every
listed row read once); the rate printed here divides it by the whole call's
time. For the kernels' own times run `--arm kernel --iters N` under
rocprofv3 --kernel-trace --stats.

    python tools/list_metrics_ab.py [--out profiles/list_metrics_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "real-time-recommendation-system-with-feature-store_amd"))

KS = [10, 100]
SHAPES = {
    "ml1m": dict(n_rows=6040, list_len=100, n_items=3900, d=64, dtype=torch.float32),
    "large": dict(n_rows=65536, list_len=100, n_items=1_000_000, d=128, dtype=torch.float16),
}


def make_inputs(shape, dev):
    g = torch.Generator(device="cpu").manual_seed(shape["n_rows"])
    emb = torch.randn(shape["n_items"], shape["d"], generator=g).to(shape["dtype"]).to(dev)
    # full lists of uniformly drawn items (a repeat within a list is allowed by both arms)
    rows = []
    for r0 in range(0, shape["n_rows"], 4096):
        n = min(4096, shape["n_rows"] - r0)
        rows.append(torch.randint(0, shape["n_items"], (n, shape["list_len"]), generator=g))
    preds = torch.cat(rows).to(dev)
    counts = torch.randint(1, 5000, (shape["n_items"],), generator=g).to(dev)
    return preds, emb, counts


def arm_kernel(preds, emb, info, default):
    from rtrec_amd.evaluation import list_metrics_tensors
    res = list_metrics_tensors(preds, KS, item_embeddings=emb, item_info=info, default_info=default)
    return res.diversity, res.novelty


def arm_torch(preds, emb, info, default):
    n, L = preds.shape
    g = emb.index_select(0, preds.reshape(-1)).view(n, L, -1).float()
    gh = g / (g.norm(dim=2, keepdim=True) + 1e-8)
    sim = torch.bmm(gh, gh.transpose(1, 2))
    div, nov = {}, {}
    for k in KS:
        kk = min(k, L)
        iu = torch.triu_indices(kk, kk, 1, device=preds.device)
        div[k] = float((1.0 - sim[:, iu[0], iu[1]]).mean(dim=1).mean().item())
        nov[k] = float(info.index_select(0, preds[:, :kk].reshape(-1)).mean().item())
    return div, nov


def timed(fn, args, window):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn(*args)
        n += 1
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if t >= window and n >= 3:
            return 1e3 * t / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,large")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--arm", choices=["both", "kernel"], default="both")
    ap.add_argument("--iters", type=int, default=0, help="with --arm kernel: run this many calls and exit (for a trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("list_metrics_ab: no GPU; nothing is measured without one")
    from rtrec_amd.evaluation import self_information
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for name in a.shapes.split(","):
        shape = SHAPES[name]
        preds, emb, counts = make_inputs(shape, dev)
        info, default = self_information(counts)
        args = (preds, emb, info, default)
        gather_bytes = shape["n_rows"] * shape["list_len"] * shape["d"] * emb.element_size()
        say(f"shape {name}: {shape['n_rows']} lists x {shape['list_len']}, table {shape['n_items']} x {shape['d']} "
            f"{str(shape['dtype']).replace('torch.', '')}; gather byte model {gather_bytes / 1e6:.1f} MB")
        if a.arm == "kernel" and a.iters > 0:
            for _ in range(a.iters):
                arm_kernel(*args)
            torch.cuda.synchronize()
            say(f"  kernel arm: {a.iters} calls done")
            continue
        dk, nk_ = arm_kernel(*args)     # warm-up of both arms, and their agreement
        arms = {"kernel": arm_kernel}
        if a.arm == "both":
            dt, nt = arm_torch(*args)
            arms["torch"] = arm_torch
            for k in KS:
                say(f"  k={k}: diversity kernel {dk[k]:.12f} torch(fp32) {dt[k]:.12f}; "
                    f"novelty kernel {nk_[k]:.12f} torch {nt[k]:.12f}")
        ms = {n: [] for n in arms}
        for _ in range(a.rounds):
            for n, fn in arms.items():   # arms alternate inside the round
                t, calls = timed(fn, args, a.window)
                ms[n].append(t)
        say("  ms per call         " + "  ".join(f"round {i + 1:<4}" for i in range(a.rounds)) + "  mean       range")
        stat = {}
        for n, v in ms.items():
            mean, rng = sum(v) / len(v), max(v) - min(v)
            stat[n] = (mean, rng)
            say(f"  {n:<18}  " + "  ".join(f"{x:<10.4f}" for x in v) + f"  {mean:<9.4f}  {rng:.4f}")
        km = stat["kernel"][0]
        say(f"  kernel arm gather rate over the whole call: {gather_bytes / (km * 1e-3) / 1e9:.1f} GB/s")
        if "torch" in stat:
            below = all(x < y for x, y in zip(ms["kernel"], ms["torch"]))
            diff = stat["torch"][0] - km
            bar = 5.0 * max(stat["kernel"][1], stat["torch"][1])
            say(f"  kernel below torch in every round: {below}; mean difference {diff:.4f} ms against "
                f"5 x {bar / 5.0:.4f} = {bar:.4f} ms: {'reached' if below and diff > bar else 'NOT reached'}; "
                f"ratio {stat['torch'][0] / km:.1f}x")
        say()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
