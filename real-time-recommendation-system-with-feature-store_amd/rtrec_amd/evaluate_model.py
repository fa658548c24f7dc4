"""Offline evaluation entry (reference scripts/evaluate_model.py:237-362).

Same arguments and flow as the reference CLI: prepare the evaluation data
(train items per user to exclude, positive test items as ground truth, the
user / movie feature tables), load the checkpoint (architecture inferred from
its weight shapes), masked top-max(k) recommendations for every test user,
``Evaluator.evaluate``, JSON results. Every step after loading runs on the
MI355X (``generate_recommendations`` → rt_exclusion_bitmap + rt_flatip_topk,
metrics → rt_rank_metrics). ``diversity@10`` / ``novelty@10``
(evaluate_model.py:309-338, metrics.py:402-478) come from ``beyond_accuracy``:
the same device ids, the model's item embeddings and a ``bincount`` of the
training interactions go to rt_list_metrics; the ranking is copied to the host
once, for the dict the Evaluator takes. Without ``ml-1m/ratings.dat``
(not shipped with the reference) the seeded ML-1M-shaped stream is used.

``--index-type hip_ivf`` (with ``--index-factory`` / ``--nprobe``) evaluates the
lists an index would serve instead of the exact ones — the reference's default
index is ``"IVF1024,Flat"`` with ``nprobe = 20`` — and adds a ``retrieval`` block
to the results: index type, nlist, nprobe and recall@k of the index's lists
against the exact lists for every k of ``--k-values``.

``--mmr-lambda`` (with ``--mmr-candidates``) evaluates the lists the MMR
re-rank would serve — the ranking stage of the request path
(src/serving/service.py:204-228): the device-resident top ``mmr_candidates`` are
re-ranked into the max(k) lists by ``rt_mmr_rerank`` before any metric, and both
values are recorded in the results next to ``diversity@10`` / ``novelty@10``.
Off by default: without the flags the results are what they were.

    python -m rtrec_amd.evaluate_model --checkpoint models/checkpoints/two_tower_best.pth
"""
from __future__ import annotations

import argparse
import json
import logging
import time
from pathlib import Path
from typing import List, Optional

import numpy as np

logger = logging.getLogger("rtrec_amd.evaluate_model")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Evaluate Two-Tower model (MI355X)")
    p.add_argument("--checkpoint", type=str, default="models/checkpoints/two_tower_best.pth")
    p.add_argument("--data-path", type=str, default="ml-1m")
    p.add_argument("--output", type=str, default="results/evaluation_results.json")
    p.add_argument("--device", type=str, default="auto")
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--k-values", type=str, default="5,10,20,50,100")
    p.add_argument("--synthetic", action="store_true", help="seeded ML-1M-shaped stream (default if ratings.dat is absent)")
    p.add_argument("--index-type", type=str, default="exact",
                   help="'exact' (default: the masked exact top-k) or a registered index type, e.g. hip_ivf: the "
                        "recommendations are that index's, and the results gain a 'retrieval' block")
    p.add_argument("--index-factory", type=str, default=None, help="the index's factory string (hip_ivf: IVF1024,Flat)")
    p.add_argument("--nprobe", type=int, default=None, help="lists probed per user (hip_ivf: 20)")
    p.add_argument("--mmr-lambda", type=float, default=None,
                   help="re-rank the top --mmr-candidates into the max(k) lists by Maximal Marginal Relevance "
                        "(0..1: the weight of the score against the similarity to what is already chosen); off by default")
    p.add_argument("--mmr-candidates", type=int, default=None,
                   help="candidates per user of the re-rank (default min(10 * max(k), 128, items); at most 128)")
    return p


def index_config_from_args(args) -> Optional[dict]:
    """The ``index_config`` of ``generate_recommendations`` for the CLI's index options (None: exact)."""
    if getattr(args, "index_type", "exact") in (None, "exact"):
        return None
    cfg = {"index_type": args.index_type}
    if args.index_factory is not None:
        cfg["index_factory"] = args.index_factory
    if args.nprobe is not None:
        cfg["nprobe"] = int(args.nprobe)
    return cfg


def retrieval_recall(index_ids, exact_ids, k_values) -> dict:
    """recall@k of an index's lists against the exact lists (device int64 [U, top_k],
    -1 = no item): per user |index[:k] ∩ exact[:k]| / |exact[:k]|, averaged over the
    users whose exact list holds an item."""
    got, want = index_ids.cpu().numpy(), exact_ids.cpu().numpy()
    out = {}
    for k in k_values:
        tot, users = 0.0, 0
        for g, w in zip(got[:, :k], want[:, :k]):
            w = set(int(i) for i in w if i >= 0)
            if w:
                tot += len(w & set(int(i) for i in g if i >= 0)) / len(w)
                users += 1
        out[f"recall@{k}"] = tot / users if users else 1.0
    return out


def prepare_evaluation_data(data):
    """evaluate_model.py:98-159: train items per user (exclusion), positive
    (label 1) test items per user (ground truth), full feature tables."""
    from .data.movielens import create_movie_features, create_user_features, get_user_positive_items
    train_items = get_user_positive_items(data.train_interactions)
    test = data.test_interactions
    pos = test[test["label"] == 1]
    test_ground_truth = {int(u): set(g["movie_idx"].tolist()) for u, g in pos.groupby("user_idx")}
    max_user = max(data.users["user_idx"].max(), data.train_interactions["user_idx"].max())
    max_movie = max(data.movies["movie_idx"].max(), data.train_interactions["movie_idx"].max())
    uf = create_user_features(data.users, np.arange(max_user + 1), normalize=True)
    mf = create_movie_features(data.movies, np.arange(max_movie + 1), normalize=True)
    return train_items, test_ground_truth, uf, mf


def beyond_accuracy(model, ids, movie_features, train_movie_idx, k: int = 10) -> dict:
    """evaluate_model.py:309-331 on the device: ``diversity@k`` of the ranking
    ``ids`` [U, top_k] (device int64, -1 = no item) over the model's own item
    embeddings, and ``novelty@k`` against the popularity of the training
    interactions (one count per ``train_movie_idx`` entry, the reference's
    ``value_counts``). Neither the ids nor the embeddings visit the host."""
    import torch

    from .evaluation import list_metrics_tensors, self_information
    dev = ids.device
    mf = torch.as_tensor(np.asarray(movie_features, np.float32)) if not isinstance(movie_features, torch.Tensor) \
        else movie_features
    with torch.no_grad():
        item_emb = model.get_item_embeddings({"numerical": mf.to(dev), "categorical": {}})
    idx = torch.as_tensor(np.asarray(train_movie_idx, np.int64)) if not isinstance(train_movie_idx, torch.Tensor) \
        else train_movie_idx
    counts = torch.bincount(idx.to(dev).to(torch.int64), minlength=int(mf.shape[0]))
    info, default = self_information(counts)
    res = list_metrics_tensors(ids, [int(k)], item_embeddings=item_emb.detach().contiguous(), item_info=info,
                               default_info=default)
    return {f"diversity@{k}": res.diversity[int(k)], f"novelty@{k}": res.novelty[int(k)]}


def run(args) -> dict:
    from .evaluation import Evaluator, generate_recommendations, load_model, recommendations_from_ids
    from .train_movielens import load_data
    k_values = [int(k) for k in args.k_values.split(",")]
    data, source = load_data(argparse.Namespace(data_path=args.data_path, synthetic=args.synthetic))
    train_items, gt, uf, mf = prepare_evaluation_data(data)
    device = None if args.device == "auto" else args.device
    model = load_model(args.checkpoint, user_dim=uf.shape[1], item_dim=mf.shape[1], device=device)
    test_users = list(gt.keys())
    t0 = time.time()
    index_config, index_info = index_config_from_args(args), {}
    mmr = {}
    if getattr(args, "mmr_lambda", None) is not None or getattr(args, "mmr_candidates", None) is not None:
        mmr = {"mmr_lambda": args.mmr_lambda, "mmr_candidates": args.mmr_candidates}
    _, ids = generate_recommendations(model, test_users, train_items, uf, mf, top_k=max(k_values),
                                      batch_size=args.batch_size, device=device, return_tensors=True,
                                      index_config=index_config, index_info=index_info, **mmr)
    recs = recommendations_from_ids(ids, test_users)
    t_recs = time.time() - t0
    retrieval = None
    if index_config is not None:
        # what the index costs: its lists against the exact ones, for the same users and exclusions
        _, exact_ids = generate_recommendations(model, test_users, train_items, uf, mf, top_k=max(k_values),
                                                batch_size=args.batch_size, device=device, return_tensors=True,
                                                **mmr)
        retrieval = {**index_info, **retrieval_recall(ids, exact_ids, k_values)}
    evaluator = Evaluator(k_values=k_values, num_items=mf.shape[0])
    metrics = evaluator.evaluate(recs, gt, exclude_items=train_items)
    results = metrics.to_dict()
    # diversity / novelty of the same device ids (k fixed at 10, evaluate_model.py:320-328)
    results.update(beyond_accuracy(model, ids, mf, data.train_interactions["movie_idx"].to_numpy(), k=10))
    results.update({"num_test_users": len(test_users), "num_items": int(mf.shape[0]), "checkpoint": args.checkpoint,
                    "data": source, "recommendation_seconds": t_recs})
    if mmr:   # next to diversity@10 / novelty@10, which they move
        from .evaluation.offline import _mmr_candidates
        results.update({"mmr_lambda": float(args.mmr_lambda),
                        "mmr_candidates": _mmr_candidates(max(k_values), args.mmr_lambda, args.mmr_candidates,
                                                          int(mf.shape[0]))})
    if retrieval is not None:
        results["retrieval"] = retrieval
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=2))
    return {"metrics": metrics, "results": results, "recommendations": recs}


def main(argv: Optional[List[str]] = None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(name)s: %(message)s")
    res = run(build_parser().parse_args(argv))
    print("\n" + str(res["metrics"]))
    print(f"Diversity@10: {res['results']['diversity@10']:.4f}")
    print(f"Novelty@10:   {res['results']['novelty@10']:.4f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
