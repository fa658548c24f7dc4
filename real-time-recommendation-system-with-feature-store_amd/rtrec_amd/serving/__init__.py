"""Serving: HBM-resident exact retrieval (reference src/serving/retrieval.py) and
the resident per-request recommender (src/serving/service.py:268-302)."""
from .online import OnlineRecommender
from .retrieval import (FaissIndex, HipFlatIPIndex, HipIVFFlatIndex, IndexBase, RetrievalEngine,
                        register_index)

__all__ = ["IndexBase", "HipFlatIPIndex", "HipIVFFlatIndex", "FaissIndex", "RetrievalEngine", "register_index",
           "OnlineRecommender"]
