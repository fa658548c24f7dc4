"""Ranking metrics of the reference's offline evaluation
(src/evaluation/metrics.py:21-319) computed on the MI355X.

Same surface: ``EvaluationMetrics`` (to_dict / __str__), the per-user
functions ``recall_at_k`` … ``average_precision`` and ``Evaluator(k_values,
num_items).evaluate(predictions, ground_truth, exclude_items)`` /
``evaluate_model``. Every value comes from ``rt_rank_metrics`` (one wave per
user: exclusion filter, ranks by ballot/popcount, ground-truth membership by
binary search, the per-user sums in the reference's rank-ascending fp64 order)
and ``rt_rank_metrics_reduce`` (means over evaluated users in a fixed order,
coverage by popcount). ``evaluate_tensors`` is the device-resident form used
by ``generate_recommendations`` output (no host round trip per user).

Contract differences, stated: a prediction list may not repeat a ground-truth
item (the top-K kernels never emit duplicates; the reference would count such
a repeat once in recall but twice in NDCG), and ids must be >= 0 (-1 pads a
ragged list). Both raise ``ValueError`` in the dict path.

Beyond accuracy (metrics.py:402-478): ``compute_diversity`` and
``compute_novelty`` keep the reference's signatures (plus ``device``);
``list_metrics_tensors`` is their device-resident form for several k at once
and ``self_information`` builds the novelty table. Both come from
``rt_list_metrics`` (one wave per list, fp64, the pair sum through
‖Σ ê‖² − Σ ‖ê‖² instead of the K×K similarity matrix) and
``rt_list_metrics_reduce``. Contract differences, stated: negative ids raise
``ValueError`` (numpy would index from the end), and a float64 embedding array
is rounded to fp32 first (the kernel reads fp32 / fp16 / bf16 tables).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Set

import numpy as np
import torch

from .. import kernels


@dataclass
class EvaluationMetrics:
    """metrics.py:21-70."""
    recall: Dict[int, float] = field(default_factory=dict)
    precision: Dict[int, float] = field(default_factory=dict)
    ndcg: Dict[int, float] = field(default_factory=dict)
    hit_rate: Dict[int, float] = field(default_factory=dict)
    mrr: float = 0.0
    map_score: float = 0.0
    coverage: float = 0.0
    per_user_recall: Dict[int, List[float]] = field(default_factory=dict)
    per_user_ndcg: Dict[int, List[float]] = field(default_factory=dict)

    def to_dict(self) -> Dict[str, float]:
        result = {}
        for k, v in self.recall.items():
            result[f"recall@{k}"] = v
        for k, v in self.precision.items():
            result[f"precision@{k}"] = v
        for k, v in self.ndcg.items():
            result[f"ndcg@{k}"] = v
        for k, v in self.hit_rate.items():
            result[f"hit_rate@{k}"] = v
        result["mrr"] = self.mrr
        result["map"] = self.map_score
        result["coverage"] = self.coverage
        return result

    def __str__(self) -> str:
        lines = ["=" * 50, "Evaluation Results", "=" * 50]
        for k in sorted(self.recall.keys()):
            lines.append(f"@{k}:")
            lines.append(f"  Recall:    {self.recall[k]:.4f}")
            lines.append(f"  Precision: {self.precision[k]:.4f}")
            lines.append(f"  NDCG:      {self.ndcg[k]:.4f}")
            lines.append(f"  Hit Rate:  {self.hit_rate[k]:.4f}")
        lines.append("-" * 50)
        lines.append(f"MRR:      {self.mrr:.4f}")
        lines.append(f"MAP:      {self.map_score:.4f}")
        lines.append(f"Coverage: {self.coverage:.4f}")
        lines.append("=" * 50)
        return "\n".join(lines)


def _device(device=None) -> torch.device:
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("evaluation metrics: no ROCm device; this MI355X build has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def csr_from_sets(rows: Sequence[Optional[Iterable[int]]], device) -> tuple:
    """(offsets int64 [n+1], items int32 sorted unique) on ``device`` from one
    item collection per row (None = empty row)."""
    offs = np.zeros(len(rows) + 1, np.int64)
    parts = []
    for i, s in enumerate(rows):
        a = np.unique(np.fromiter((int(x) for x in s), np.int64)) if s is not None else np.zeros(0, np.int64)
        if a.size and (a[0] < np.iinfo(np.int32).min or a[-1] > np.iinfo(np.int32).max):
            raise ValueError("item ids must fit in int32")
        parts.append(a)
        offs[i + 1] = offs[i] + a.size
    items = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return torch.from_numpy(offs).to(device), torch.from_numpy(items).to(device)


def _pack_predictions(lists: Sequence[Sequence[int]], device) -> torch.Tensor:
    width = max([len(x) for x in lists] + [1])
    arr = np.full((len(lists), width), -1, np.int64)
    for i, x in enumerate(lists):
        if len(x):
            a = np.asarray(x, np.int64)
            if (a < 0).any():
                raise ValueError("predicted item ids must be >= 0 (-1 pads ragged lists on the device)")
            arr[i, :len(a)] = a
    return torch.from_numpy(arr).to(device)


def _check_repeats(lists, gts):
    for x, g in zip(lists, gts):
        if g is None or len(x) == len(set(x)):
            continue
        seen, rep = set(), set()
        for it in x:
            (rep if it in seen else seen).add(it)
        if rep & set(g):
            raise ValueError("a prediction list repeats a ground-truth item (unsupported; top-K output never does)")


def evaluate_tensors(preds: torch.Tensor, gt_offsets: torch.Tensor, gt_items: torch.Tensor, k_values: Sequence[int],
                     gt_rows: Optional[torch.Tensor] = None, ex_offsets: Optional[torch.Tensor] = None,
                     ex_items: Optional[torch.Tensor] = None, ex_rows: Optional[torch.Tensor] = None,
                     num_items: Optional[int] = None) -> EvaluationMetrics:
    """Evaluator.evaluate on device-resident rankings [n, L] (-1 = no item) and
    CSR ground truth / exclusions (row indirection via *_rows)."""
    ks = sorted(int(k) for k in k_values)
    per_row, valid, summary = kernels.rank_metrics(preds, gt_offsets, gt_items, ks, gt_rows=gt_rows,
                                                   ex_offsets=ex_offsets, ex_items=ex_items, ex_rows=ex_rows,
                                                   num_items=int(num_items or 0))
    return _to_metrics(per_row, valid, summary, ks)


def _to_metrics(per_row, valid, summary, ks) -> EvaluationMetrics:
    nk = len(ks)
    s = summary.cpu().numpy()
    v = valid.cpu().numpy().astype(bool)
    pr = per_row.cpu().numpy()[v]
    m = EvaluationMetrics()
    for i, k in enumerate(ks):
        m.recall[k] = float(s[i])
        m.precision[k] = float(s[nk + i])
        m.ndcg[k] = float(s[2 * nk + i])
        m.hit_rate[k] = float(s[3 * nk + i])
        m.per_user_recall[k] = pr[:, i].tolist()
        m.per_user_ndcg[k] = pr[:, 2 * nk + i].tolist()
    m.mrr = float(s[4 * nk])
    m.map_score = float(s[4 * nk + 1])
    m.coverage = float(s[4 * nk + 3])
    return m


class Evaluator:
    """metrics.py:231-399."""

    def __init__(self, k_values: List[int] = [5, 10, 20, 50, 100], num_items: Optional[int] = None,
                 device=None):
        self.k_values = sorted(k_values)
        self.num_items = num_items
        self.device = device

    def evaluate(self, predictions: Dict[int, List[int]], ground_truth: Dict[int, Set[int]],
                 exclude_items: Optional[Dict[int, Set[int]]] = None) -> EvaluationMetrics:
        """metrics.py:248-319: per-user metrics over users present in both dicts
        (empty ground truth skipped), excluded items removed from each list first."""
        dev = _device(self.device)
        users = list(predictions.keys())
        lists = [list(predictions[u]) for u in users]
        gts = [ground_truth.get(u) if u in ground_truth else None for u in users]
        _check_repeats(lists, gts)
        preds = _pack_predictions(lists, dev)
        go, gi = csr_from_sets(gts, dev)
        eo = ei = None
        if exclude_items:
            eo, ei = csr_from_sets([exclude_items.get(u) for u in users], dev)
        return evaluate_tensors(preds, go, gi, self.k_values, ex_offsets=eo, ex_items=ei, num_items=self.num_items)

    def evaluate_model(self, model, test_users: List[int], test_ground_truth: Dict[int, Set[int]],
                       train_items: Dict[int, Set[int]], user_features: np.ndarray, item_features: np.ndarray,
                       item_ids: List[int], batch_size: int = 256, device=None) -> EvaluationMetrics:
        """metrics.py:321-399: masked top-max(k) for every test user on the device
        (generate_recommendations), mapped through ``item_ids``, then evaluate."""
        from .offline import generate_recommendations
        model.eval()
        recs = generate_recommendations(model, test_users, train_items, user_features, item_features,
                                        top_k=max(self.k_values), batch_size=batch_size, device=device)
        ids = list(item_ids)
        predictions = {u: [ids[i] for i in recs[u]] for u in test_users}
        return self.evaluate(predictions, test_ground_truth)


@dataclass
class ListMetrics:
    """Result of ``list_metrics_tensors``: per-k summaries on the host, per-row
    diversity on the device."""
    diversity: Dict[int, float] = field(default_factory=dict)
    novelty: Dict[int, float] = field(default_factory=dict)
    per_row_diversity: Optional[torch.Tensor] = None   # fp64 [n_rows, n_k], 0 where not valid
    diversity_valid: Optional[torch.Tensor] = None     # int32 [n_rows, n_k]: the row has >= 2 items at this k
    diversity_rows: Dict[int, int] = field(default_factory=dict)    # rows averaged per k
    novelty_entries: Dict[int, int] = field(default_factory=dict)   # list entries averaged per k


def self_information(counts, total: Optional[float] = None):
    """The novelty table of ``compute_novelty`` (metrics.py:467-476): (info fp64
    [n_info], default) with ``info[i] = -log2(pop_i / total + 1e-10)`` and
    ``default`` the value of an item the popularity table does not hold (pop 1).
    ``counts`` is the reference's ``{item: count}`` dict (a host table comes
    back) or a per-item count tensor such as a ``bincount`` (a zero count means
    absent; the table stays on the tensor's device). ``total`` defaults to the
    sum of the counts held; a zero total raises ``ZeroDivisionError`` as the
    reference's division does."""
    if isinstance(counts, dict):
        keys = np.fromiter((int(i) for i in counts.keys()), np.int64, len(counts))
        vals = np.fromiter((float(v) for v in counts.values()), np.float64, len(counts))
        if keys.size and keys.min() < 0:
            raise ValueError("item ids must be >= 0")
        tot = float(sum(counts.values())) if total is None else float(total)
        if tot == 0.0:
            raise ZeroDivisionError("division by zero: the item popularity table sums to 0")
        default = float(-np.log2(1.0 / tot + 1e-10))
        info = np.full(int(keys.max()) + 1 if keys.size else 0, default, np.float64)
        info[keys] = -np.log2(vals / tot + 1e-10)
        return torch.from_numpy(info), default
    c = torch.as_tensor(counts)
    if c.dim() != 1:
        raise ValueError("a count tensor must be 1-D, one count per item")
    c = c.to(torch.float64)
    tot = float(c.sum().item()) if total is None else float(total)
    if tot == 0.0:
        raise ZeroDivisionError("division by zero: the item popularity table sums to 0")
    pop = torch.where(c > 0, c, torch.ones_like(c))
    return -torch.log2(pop / tot + 1e-10), float(-np.log2(1.0 / tot + 1e-10))


def list_metrics_tensors(preds: torch.Tensor, k_values: Sequence[int],
                         item_embeddings: Optional[torch.Tensor] = None, item_info: Optional[torch.Tensor] = None,
                         default_info: Optional[float] = None) -> ListMetrics:
    """compute_diversity / compute_novelty on device-resident rankings [n, L]
    (-1 = no item) for every k of ``k_values`` in one pass. ``item_embeddings``
    [num_items, d] fp32 / fp16 / bf16 and ``item_info`` / ``default_info`` (from
    ``self_information``) are each optional; a metric without its operand is
    left out of the result."""
    if item_info is not None and default_info is None:
        raise ValueError("item_info needs default_info (self_information returns both)")
    ks = sorted(int(k) for k in k_values)
    div, valid, _, _, summary = kernels.list_metrics(preds, ks, emb=item_embeddings, info=item_info,
                                                     default_info=0.0 if default_info is None else default_info)
    s = summary.cpu().numpy()
    out = ListMetrics(per_row_diversity=div, diversity_valid=valid)
    for i, k in enumerate(ks):
        if item_embeddings is not None:
            out.diversity[k] = float(s[0, i])
            out.diversity_rows[k] = int(s[1, i])
        if item_info is not None:
            out.novelty[k] = float(s[2, i])
            out.novelty_entries[k] = int(s[3, i])
    return out


def _embedding_table(item_embeddings, dev) -> torch.Tensor:
    if isinstance(item_embeddings, torch.Tensor):
        t = item_embeddings.detach()
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            t = t.to(torch.float32)
        return t if t.device.type == "cuda" else t.to(dev)
    return torch.from_numpy(np.ascontiguousarray(item_embeddings, dtype=np.float32)).to(dev)


def _list_device(device, *tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.device.type == "cuda":
            return t.device  # a device tensor is used where it lies
    return _device(device)


def compute_diversity(recommendations: Dict[int, List[int]], item_embeddings, k: int = 10, device=None) -> float:
    """metrics.py:402-446: mean over users with at least two items in their first
    ``k`` of the mean pairwise cosine distance ``1 - ê_i·ê_j``, ``ê = e / (‖e‖ +
    1e-8)``; 0.0 when no user qualifies. ``item_embeddings`` is a numpy array
    or a tensor (a device tensor is used in place). Ids past the table raise
    ``IndexError`` as numpy does; negative ids raise ``ValueError``."""
    dev = _list_device(device, item_embeddings)
    lists = [list(x)[:int(k)] for x in recommendations.values()]
    if not lists:
        return 0.0
    res = list_metrics_tensors(_pack_predictions(lists, dev), [int(k)],
                               item_embeddings=_embedding_table(item_embeddings, dev))
    return res.diversity[int(k)]


def compute_novelty(recommendations: Dict[int, List[int]], item_popularity: Dict[int, int], k: int = 10,
                    device=None) -> float:
    """metrics.py:449-478: flat mean over every entry of every user's first ``k``
    of ``-log2(pop / total + 1e-10)``, ``pop`` the item's count (1 for an item
    ``item_popularity`` does not hold) and ``total`` the sum of the counts; 0.0
    without entries. An all-zero or empty table with non-empty lists raises
    ``ZeroDivisionError``."""
    dev = _list_device(device)
    lists = [list(x)[:int(k)] for x in recommendations.values()]
    if not any(len(x) for x in lists):
        return 0.0
    info, default = self_information(dict(item_popularity))
    res = list_metrics_tensors(_pack_predictions(lists, dev), [int(k)], item_info=info.to(dev), default_info=default)
    return res.novelty[int(k)]


def _single(predicted: List[int], ground_truth: Set[int], k: int):
    """Per-row values of one user (one rt_rank_metrics row)."""
    dev = _device()
    _check_repeats([list(predicted)], [ground_truth])
    preds = _pack_predictions([list(predicted)], dev)
    go, gi = csr_from_sets([ground_truth], dev)
    per_row, _, _ = kernels.rank_metrics(preds, go, gi, [int(k)])
    return per_row[0].cpu().numpy()


def recall_at_k(predicted: List[int], ground_truth: Set[int], k: int) -> float:
    """metrics.py:73-96."""
    return float(_single(predicted, ground_truth, k)[0])


def precision_at_k(predicted: List[int], ground_truth: Set[int], k: int) -> float:
    """metrics.py:99-119 (hits / k even for an empty ground truth: 0)."""
    return float(_single(predicted, ground_truth, k)[1])


def ndcg_at_k(predicted: List[int], ground_truth: Set[int], k: int) -> float:
    """metrics.py:122-157."""
    return float(_single(predicted, ground_truth, k)[2])


def hit_rate_at_k(predicted: List[int], ground_truth: Set[int], k: int) -> float:
    """metrics.py:160-178."""
    return float(_single(predicted, ground_truth, k)[3])


def reciprocal_rank(predicted: List[int], ground_truth: Set[int]) -> float:
    """metrics.py:181-199."""
    return float(_single(predicted, ground_truth, 1)[4])


def average_precision(predicted: List[int], ground_truth: Set[int]) -> float:
    """metrics.py:202-228."""
    return float(_single(predicted, ground_truth, 1)[5])
