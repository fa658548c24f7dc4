"""Offline evaluation caller of the top-K path (reference scripts/evaluate_model.py).

``generate_recommendations`` (evaluate_model.py:162-234): all item embeddings
once, the user tower over the test users in ``batch_size`` batches, then per
user the train items masked out and the top ``top_k`` items by inner product.
The reference does the last step as ``np.dot`` + ``-inf`` masking + a full-row
``argsort`` (≈299 ms for 6,040 × 3,416 on the survey host); here it is one
``rt_flatip_topk`` launch with the train-item exclusion bitmap built on the
device (``rt_exclusion_bitmap``) from a CSR of the train items — no score
matrix is materialised.

Ordering: (score desc, item id asc). The reference's ``argsort(...)[::-1]``
orders exact score ties by a quicksort-dependent rule; outside exact ties the
lists are identical (tests/test_gpu_eval.py checks this tie-aware against the
reference's own output, tests/golden/eval_topk.npz). When a user has fewer
than ``top_k`` non-train items the reference appends its ``-inf`` train items
in argsort order; by default this build returns only the eligible items (the
reference's Evaluator removes those train items again before scoring,
metrics.py:279-281). ``pad_excluded=True`` returns the reference's full-length
lists instead: such a user's top_k already holds every eligible item with its
score, so the masked score row is known exactly, and the list is
``np.argsort(row)[::-1][:top_k]`` over it — the reference's own call
(evaluate_model.py:225-231), whose order among the ``-inf`` ties is numpy's
(its introsort/SIMD sort is not stable, so no other rule reproduces it).

``load_model`` (evaluate_model.py:36-95): architecture inferred from the
checkpoint's weight shapes, ``weights_only=True``.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import kernels
from ..models.two_tower import ItemTower, TwoTowerModel, UserTower
from .metrics import csr_from_sets


def _dev(device) -> torch.device:
    if device in (None, "auto", "cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("generate_recommendations: no ROCm device; this MI355X build has no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def build_eval_index(item_emb: torch.Tensor, index_config: Dict[str, Any]):
    """The item embeddings built into a registered index class (``index_type``,
    default ``"hip_ivf"``; the other keys are the class's own: ``index_factory``,
    ``nprobe``, ``storage_dtype`` ...). ``metric`` is forced to
    ``"inner_product"``, so scores stay the towers' dot products, and
    ``batch_min_queries`` defaults to 1: an evaluation searches thousands of
    users in one call, the shape the list-major scan is for. Positions are the
    item ids."""
    from ..serving import retrieval
    cfg = dict(index_config)
    index_type = cfg.pop("index_type", "hip_ivf")
    cls = retrieval._INDEX_TYPES.get(index_type)
    if cls is None or not hasattr(cls, "search_tensors"):
        raise ValueError(f"index_type={index_type!r}: not a registered device index "
                         f"(one of {sorted(n for n, c in retrieval._INDEX_TYPES.items() if hasattr(c, 'search_tensors'))})")
    cfg.setdefault("batch_min_queries", 1)
    cfg["metric"] = "inner_product"
    cfg["dimension"] = int(item_emb.shape[1])
    index = cls(cfg)
    index.build(item_emb, [str(i) for i in range(item_emb.shape[0])])
    return index


@torch.no_grad()
def recommend_tensors(model: TwoTowerModel, user_features: torch.Tensor, item_features: torch.Tensor,
                      test_users: torch.Tensor, train_offsets: torch.Tensor, train_items: torch.Tensor,
                      top_k: int = 100, batch_size: int = 256, index_config: Optional[Dict[str, Any]] = None,
                      index_info: Optional[Dict[str, Any]] = None, mmr_lambda: Optional[float] = None,
                      mmr_candidates: Optional[int] = None):
    """Device-resident form: ``user_features`` [n_users, Fu] / ``item_features``
    [n_items, Fi] fp32 tables, ``test_users`` int64 [U], train items as a CSR
    over user rows. Returns (scores fp32 [U, top_k], item ids int64 [U, top_k]),
    (-FLT_MAX, -1) where fewer than top_k items are eligible.

    ``index_config``: search through an index instead of exactly — the item
    embeddings are built into :func:`build_eval_index`'s index and the users
    searched with ``index.search_tensors(user_emb, top_k, exclude_bits=bits)``,
    so the lists are what a deployment with that index (the default
    ``"IVF1024,Flat"``, ``nprobe = 20``) would serve; ``top_k`` above the
    index's limit raises the index's own error. ``index_info`` (a dict) is
    filled with the index type, nlist and nprobe used.

    ``mmr_lambda`` (None = off; in [0, 1]) / ``mmr_candidates`` (default
    ``min(10 * top_k, 128, n_items)``; top_k <= mmr_candidates <= 128): the lists
    are the MMR re-rank (``rt_mmr_rerank``, cosine similarities of the item
    embeddings) of the device-resident top ``mmr_candidates`` — exact, or the
    index's — into ``top_k``, in selection order with the original scores; with
    and without ``index_config``."""
    n_cand = _mmr_candidates(top_k, mmr_lambda, mmr_candidates, int(item_features.shape[0]))
    k_search = n_cand or top_k
    item_emb = model.get_item_embeddings({"numerical": item_features, "categorical": {}})
    n_items = item_emb.shape[0]
    u_idx = test_users.to(torch.int64)
    parts = []
    for i in range(0, u_idx.numel(), batch_size):  # evaluate_model.py:201-215 (eval BN: batching is exact)
        uf = kernels.gather_rows(user_features, u_idx[i:i + batch_size], check=True)
        parts.append(model.get_user_embeddings({"numerical": uf, "categorical": {}}))
    user_emb = torch.cat(parts) if len(parts) != 1 else parts[0]
    bits = kernels.exclusion_bitmap_csr(train_offsets, train_items, n_items, rows=u_idx)
    if index_config is not None:
        index = build_eval_index(item_emb.contiguous(), index_config)
        if index_info is not None:
            fallback = getattr(index, "_flat", None) is not None   # a corpus too small for IVF lists
            nlist = None if fallback else getattr(index, "nlist", None)
            index_info.update({"index_type": index_config.get("index_type", "hip_ivf"), "nlist": nlist,
                               "nprobe": None if nlist is None else index._n_probe()})
        scores, ids = index.search_tensors(user_emb.contiguous(), k_search, exclude_bits=bits)
        return index.mmr_rerank_tensors(scores, ids, top_k, mmr_lambda) if n_cand else (scores, ids)
    item_emb = item_emb.contiguous()
    scores, ids = kernels.flatip_topk(user_emb.contiguous(), item_emb, k_search, exclude_bits=bits)
    if n_cand:
        return kernels.mmr_rerank(scores, ids, item_emb, top_k, mmr_lambda, normalize=True)
    return scores, ids


def _mmr_candidates(top_k: int, mmr_lambda: Optional[float], mmr_candidates: Optional[int], n_items: int) -> int:
    """The candidates per user of a re-ranked evaluation (0: off), with the bounds of
    ``HipFlatIPIndex.search``: 0 <= mmr_lambda <= 1, top_k <= mmr_candidates <= 128."""
    if mmr_lambda is None:
        if mmr_candidates is not None:
            raise ValueError("mmr_candidates without mmr_lambda: the re-rank is off (mmr_lambda=None)")
        return 0
    if not 0.0 <= float(mmr_lambda) <= 1.0:
        raise ValueError(f"mmr_lambda={mmr_lambda}: 0 <= mmr_lambda <= 1")
    cap = kernels.MMR_MAX_CAND
    if mmr_candidates is None:
        mmr_candidates = max(min(10 * top_k, cap, n_items), min(top_k, cap))
    if not top_k <= int(mmr_candidates) <= cap:
        raise ValueError(f"mmr_candidates={mmr_candidates}: top_k <= mmr_candidates <= {cap} (top_k={top_k})")
    return int(mmr_candidates)


def _pad_like_reference(ids_row: np.ndarray, scores_row: np.ndarray, n_items: int, top_k: int) -> List[int]:
    """A user with fewer than top_k eligible items: rebuild the reference's masked
    score row (eligible items' scores, -inf elsewhere) and take its argsort,
    as scripts/evaluate_model.py:225-231 does."""
    ok = ids_row >= 0
    row = np.full(n_items, -np.inf, dtype=np.float32)
    row[ids_row[ok]] = scores_row[ok]
    return [int(x) for x in np.argsort(row)[::-1][:top_k]]


def recommendations_from_ids(ids: torch.Tensor, users: Sequence[int]) -> Dict[int, List[int]]:
    """Dict[user_idx, List[movie_idx]] from device ids [U, top_k] (row r belongs to
    ``users[r]``; -1 = no item): the one host copy of a ranking."""
    host = ids.cpu().numpy()
    return {int(u): [int(x) for x in host[r] if x >= 0] for r, u in enumerate(users)}


def generate_recommendations(model: TwoTowerModel, test_users: list, train_items: Dict[int, list],
                             user_features: np.ndarray, movie_features: np.ndarray, top_k: int = 100,
                             batch_size: int = 256, device: Optional[str] = None,
                             return_tensors: bool = False, pad_excluded: bool = False,
                             index_config: Optional[Dict[str, Any]] = None,
                             index_info: Optional[Dict[str, Any]] = None, mmr_lambda: Optional[float] = None,
                             mmr_candidates: Optional[int] = None):
    """evaluate_model.py:162-234 → Dict[user_idx, List[movie_idx]] (or the
    device (scores, ids) with ``return_tensors``). ``pad_excluded``: lists of
    users with fewer than ``top_k`` eligible items are padded with their
    excluded items as the reference pads them (see the module docstring).
    ``index_config`` / ``index_info``: as :func:`recommend_tensors` — the lists
    of an index (``{"index_type": "hip_ivf", "index_factory": "IVF1024,Flat",
    "nprobe": 20}``) instead of the exact ones; without it nothing changes.
    ``mmr_lambda`` / ``mmr_candidates``: as :func:`recommend_tensors` — the lists are
    the MMR re-rank of the top ``mmr_candidates`` into ``top_k``; off by default."""
    dev = _dev(device)
    uf = torch.as_tensor(np.asarray(user_features, np.float32)).to(dev)
    mf = torch.as_tensor(np.asarray(movie_features, np.float32)).to(dev)
    users = [int(u) for u in test_users]
    n_users = uf.shape[0]
    rows: List[Optional[Sequence[int]]] = [None] * n_users
    for u, its in train_items.items():
        if 0 <= int(u) < n_users:
            rows[int(u)] = its
    t_off, t_items = csr_from_sets(rows, dev)
    scores, ids = recommend_tensors(model, uf, mf, torch.tensor(users, dtype=torch.int64, device=dev), t_off,
                                    t_items, top_k=top_k, batch_size=batch_size, index_config=index_config,
                                    index_info=index_info, mmr_lambda=mmr_lambda, mmr_candidates=mmr_candidates)
    if return_tensors:
        return scores, ids
    if not pad_excluded:
        return recommendations_from_ids(ids, users)
    host = ids.cpu().numpy()
    n_items = mf.shape[0]
    host_s = scores.cpu().numpy()
    out = {}
    for r, u in enumerate(users):
        if top_k <= n_items and (host[r] < 0).any():
            out[u] = _pad_like_reference(host[r], host_s[r], n_items, top_k)
        else:
            out[u] = [int(x) for x in host[r] if x >= 0]
    return out


def load_model(checkpoint_path: str, user_dim: int, item_dim: int, device: Optional[str] = None) -> TwoTowerModel:
    """evaluate_model.py:36-95: hidden sizes from mlp.0 / mlp.4, embedding dim from
    mlp.8 (two hidden layers, as the reference infers), dropout 0.2, ReLU, no
    content projection, biases not restored (the reference ignores them)."""
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    us = ck["user_tower_state"]
    hidden = [us["mlp.0.weight"].shape[0], us["mlp.4.weight"].shape[0]]
    emb = us["mlp.8.weight"].shape[0]
    ut = UserTower(input_dim=user_dim, embedding_dim=emb, hidden_layers=hidden, dropout_rate=0.2, activation="relu")
    it = ItemTower(input_dim=item_dim, embedding_dim=emb, hidden_layers=hidden, dropout_rate=0.2, activation="relu",
                   use_content_embedding=False)
    model = TwoTowerModel(user_tower=ut, item_tower=it, temperature=ck.get("temperature", 0.1), use_bias=True)
    model.user_tower.load_state_dict(ck["user_tower_state"])
    model.item_tower.load_state_dict(ck["item_tower_state"])
    model.to(_dev(device))
    model.eval()
    return model
