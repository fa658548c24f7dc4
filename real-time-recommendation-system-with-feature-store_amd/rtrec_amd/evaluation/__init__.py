"""Offline evaluation on the MI355X (reference src/evaluation/metrics.py and
scripts/evaluate_model.py)."""
from .metrics import (EvaluationMetrics, Evaluator, ListMetrics, average_precision, compute_diversity,  # noqa: F401
                      compute_novelty, evaluate_tensors, hit_rate_at_k, list_metrics_tensors, ndcg_at_k,
                      precision_at_k, recall_at_k, reciprocal_rank, self_information)
from .offline import (generate_recommendations, load_model, recommend_tensors,  # noqa: F401
                      recommendations_from_ids)
