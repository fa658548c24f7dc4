"""Resident recommender: user features (or user ids) in, recommendation lists
out, with ONE graph replay and ONE synchronise per request.

It replaces the reference's per-request pair (src/serving/service.py:268-302:
``model.get_user_embeddings(one row)`` → ``.cpu().numpy()`` →
``RetrievalEngine.retrieve``, src/serving/retrieval.py:561-627) — a chain of
one launch per Linear, two synchronises and a host round trip of the
embedding — by ``rt_tower_infer_f32`` (the whole eval-mode tower for 1..8 rows
in one launch) composed with :class:`~rtrec_amd.serving.retrieval.OnlineSearcher`'s
device chain. Importing this module touches no device.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import kernels, native
from ..models.fused import blocks_from_sequential
from .retrieval import HipFlatIPIndex, OnlineSearcher, RetrievalEngine, _capture, _lists_from_positions

Features = Union[np.ndarray, torch.Tensor, Dict[str, Any]]
Rows = Union[np.ndarray, torch.Tensor]


class NoDeviceError(ValueError, RuntimeError):
    """A model, table or index that is not on a ROCm device. A ``ValueError``
    like every refusal at construction, and a ``RuntimeError`` like every other
    "no CPU fallback" refusal of the package (``native.require_device``)."""


class OnlineRecommender:
    """``OnlineRecommender(model, index, max_batch=8, user_table=None)``.

    ``model``: a :class:`~rtrec_amd.models.two_tower.TwoTowerModel` (its user
    tower is served) or a tower. ``index``: a :class:`HipFlatIPIndex`, or a
    :class:`RetrievalEngine` whose index is one. ``user_table``: an optional
    resident ``[n_users, F]`` fp32 device tensor (the MovieLens user table
    ``evaluation/offline.py`` gathers from); ``user_ids`` are its rows.

    **Eval semantics hold regardless of** ``model.training``: BatchNorm uses
    its running statistics and dropout is off, as in the serving path
    (service.py:286-293 runs under ``model.eval()``).

    Everything is allocated at construction: pinned host buffers for features /
    ids / embedding (scores / positions are the searcher's), their device
    twins, and the 4 MiB top-K workspace. A call copies into a pinned buffer,
    replays a graph captured lazily per ``(nq, k_search, by_ids)`` and
    synchronises once. The graph is a straight chain: H2D copy →
    ``rt_tower_infer_f32`` → D2H copy of the embedding → ``l2_renorm`` (cosine)
    → storage-dtype cast → ``rt_flatip_topk_online`` → D2H copies of scores and
    positions; from the renorm on it is ``OnlineSearcher._device_chain``, so
    ``recommend(x, k)`` returns what ``index.search(embed(x), k)`` returns
    through the online searcher. ``embed`` replays H2D → tower → D2H.
    ``RTREC_ONLINE_GRAPH=0`` (read at every call) runs the chains eagerly.

    Calls outside the graphs' range (``k_search`` > 128, more than
    ``max_batch`` rows) embed in chunks of ``max_batch`` and call
    ``index.search``: the same lists, not resident.

    Staleness. Index: ``build`` / ``add`` / ``load`` bump its generation and
    the search graphs are dropped and captured again. Model: the graphs hold the live
    parameter and buffer tensors, so in-place changes (optimiser steps,
    ``load_state_dict``, ``load_model``) are seen by the next call; a change
    that RE-ALLOCATES them (``model.to(...)``, a rebuilt ``ParamSlab``) needs
    :meth:`refresh`. There is no per-call pointer scan. Construction and
    ``refresh`` make the model's parameter slab (what the first forward of the
    model would do), so a later forward does not move the parameters.

    Thread safety: as :class:`OnlineSearcher` — calls are serialised by the
    re-entrant ``lock``; ``embed`` returns a view of a pinned buffer, valid
    until the next call.
    """

    MAX_BATCH = native.TOWER_MAX_ROWS
    MAX_GRAPHS = 64

    def __init__(self, model: nn.Module, index: Union[HipFlatIPIndex, RetrievalEngine], max_batch: int = 8,
                 user_table: Optional[torch.Tensor] = None):
        if not 1 <= int(max_batch) <= self.MAX_BATCH:
            raise ValueError(f"max_batch={max_batch}: 1..{self.MAX_BATCH}")
        self.max_batch = int(max_batch)
        self.model = model
        self.tower = getattr(model, "user_tower", model)
        if isinstance(index, RetrievalEngine):
            index = index.index
        if not isinstance(index, HipFlatIPIndex):
            raise ValueError(f"index must be a HipFlatIPIndex (or a RetrievalEngine over one), got "
                             f"{type(index).__name__}")
        self.index = index
        # -- what rt_tower_infer_f32 serves ------------------------------------
        if len(getattr(self.tower, "embeddings", {})) or getattr(self.tower, "categorical_features", None):
            raise ValueError("OnlineRecommender serves towers without categorical embeddings (numerical features "
                             "plus an optional id gather; the service path passes categorical: {})")
        self._blocks = blocks_from_sequential(self.tower.mlp)
        if len(self._blocks) > native.TOWER_MAX_LAYERS:
            raise ValueError(f"{len(self._blocks)} Linear layers: rt_tower_infer_f32 takes at most "
                             f"{native.TOWER_MAX_LAYERS}")
        for b in self._blocks:
            if max(b.linear.in_features, b.linear.out_features) > native.TOWER_MAX_WIDTH:
                raise ValueError(f"layer width {max(b.linear.in_features, b.linear.out_features)} > "
                                 f"{native.TOWER_MAX_WIDTH}")
        self.input_dim = self._blocks[0].linear.in_features
        self.dimension = self._blocks[-1].linear.out_features
        if index.dimension != self.dimension:
            raise ValueError(f"index dimension {index.dimension} != tower embedding dimension {self.dimension}")
        if index._l2:
            raise ValueError("OnlineRecommender serves the inner-product metrics ('cosine', 'inner_product')")
        # -- devices: no CPU fallback ------------------------------------------
        p0 = self._blocks[0].linear.weight
        if p0.device.type != "cuda":
            raise NoDeviceError(f"OnlineRecommender: the model is on {p0.device}; this MI355X build has no CPU "
                                "fallback")
        try:
            dev = index._dev()
        except RuntimeError as e:
            raise NoDeviceError(str(e)) from e
        if dev.type != "cuda":
            raise NoDeviceError(f"OnlineRecommender: the index is on {dev}; this MI355X build has no CPU fallback")
        if dev.index is not None and p0.device.index is not None and dev.index != p0.device.index:
            raise ValueError(f"the model is on {p0.device}, the index on {dev}")
        dev = p0.device
        if user_table is not None:
            if user_table.device.type != "cuda":
                raise NoDeviceError(f"OnlineRecommender: user_table is on {user_table.device}; this MI355X build "
                                    "has no CPU fallback")
            if user_table.dim() != 2 or user_table.dtype != torch.float32 or user_table.shape[1] != self.input_dim \
                    or user_table.stride(1) != 1:
                raise ValueError(f"user_table must be fp32 [n_users, {self.input_dim}] with unit column stride")
        self.user_table = user_table
        native.lib()
        mb, f, d = self.max_batch, self.input_dim, self.dimension
        self._searcher = OnlineSearcher(index, mb)
        self.lock = self._searcher.lock
        self._h_x = torch.empty((mb, f), dtype=torch.float32).pin_memory()
        self._h_ids = torch.empty(mb, dtype=torch.int64).pin_memory()
        self._h_e = torch.empty((mb, d), dtype=torch.float32).pin_memory()
        self._h_x_np, self._h_ids_np, self._h_e_np = self._h_x.numpy(), self._h_ids.numpy(), self._h_e.numpy()
        self._d_x = torch.empty((mb, f), dtype=torch.float32, device=dev)
        self._d_ids = torch.empty(mb, dtype=torch.int64, device=dev)
        self._graphs: "OrderedDict[Tuple[int, int, bool], torch.cuda.CUDAGraph]" = OrderedDict()
        self._layers = None
        self.refresh()

    # -- the model's tensors ---------------------------------------------------
    def refresh(self):
        """Re-read the parameter / buffer pointers and drop the graphs: needed
        after a change that re-allocates the model's tensors."""
        with self.lock:
            self._graphs.clear()
            from ..models.two_tower import _slab_of
            _slab_of(self.tower)
            layers = (native.TowerLayer * native.TOWER_MAX_LAYERS)()
            keep: List[torch.Tensor] = []

            def p(t: Optional[torch.Tensor]):
                if t is None:
                    return None
                if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                    raise NoDeviceError(f"OnlineRecommender: a model tensor is {t.dtype} on {t.device}; the kernel "
                                        "reads contiguous fp32 device tensors (no CPU fallback)")
                keep.append(t)
                return ctypes.c_void_p(t.data_ptr())

            for i, b in enumerate(self._blocks):
                lin, L = b.linear, layers[i]
                L.w, L.bias = p(lin.weight.data), p(lin.bias.data if lin.bias is not None else None)
                L.k, L.n, L.act = lin.in_features, lin.out_features, b.act
                if b.bn is not None:
                    if b.bn.running_mean is None or b.bn.weight is None:
                        raise ValueError("BatchNorm1d without running statistics or affine parameters")
                    L.bn_gamma, L.bn_beta = p(b.bn.weight.data), p(b.bn.bias.data)
                    L.bn_mean, L.bn_var = p(b.bn.running_mean), p(b.bn.running_var)
                    L.bn_eps = float(b.bn.eps)
            self._layers, self._keep = layers, keep

    def _tower(self, nq: int, by_ids: bool):
        """Launch rt_tower_infer_f32 for ``nq`` rows into the searcher's fp32 query rows."""
        a = native.TowerInferArgs()
        if by_ids:
            t = self.user_table
            a.src, a.src_rows, a.ld_src = native.ptr(t), t.shape[0], t.stride(0)
            a.ids = native.ptr(self._d_ids)
        else:
            a.src, a.src_rows, a.ld_src = native.ptr(self._d_x), self.max_batch, self.input_dim
        a.m, a.n_layers, a.layers, a.normalize = nq, len(self._blocks), self._layers, 1
        a.out = native.ptr(self._searcher._d_q32)
        kernels.tower_infer(a, native.stream_of(self._d_x))

    def _sequence(self, nq: int, k: int, by_ids: bool):
        """The stream-ordered chain of one call (k = 0: embed only)."""
        if by_ids:
            self._d_ids[:nq].copy_(self._h_ids[:nq], non_blocking=True)
        else:
            self._d_x[:nq].copy_(self._h_x[:nq], non_blocking=True)
        self._tower(nq, by_ids)
        # the embedding leaves before the renorm rewrites the rows in place
        self._h_e[:nq].copy_(self._searcher._d_q32[:nq], non_blocking=True)
        if k:
            self._searcher._device_chain(nq, k)
            self._searcher._download(nq, k)

    # -- inputs ------------------------------------------------------------------
    def _rows_of(self, user_features: Optional[Features], user_ids) -> Tuple[Optional[Rows], Optional[np.ndarray]]:
        if (user_features is None) == (user_ids is None):
            raise ValueError("give exactly one of user_features and user_ids")
        if user_ids is not None:
            if self.user_table is None:
                raise ValueError("user_ids need the user_table the recommender was made with")
            ids = np.asarray(user_ids.cpu() if isinstance(user_ids, torch.Tensor) else user_ids).reshape(-1)
            if ids.size and not np.issubdtype(ids.dtype, np.integer):
                raise TypeError("user_ids must be integers")
            ids = ids.astype(np.int64, copy=False)
            n_users = self.user_table.shape[0]
            if ids.size and (ids.min() < 0 or ids.max() >= n_users):
                raise IndexError(f"user id out of range for a table of {n_users} rows")
            return None, ids
        x = user_features
        if isinstance(x, dict):
            if x.get("categorical"):
                raise ValueError("OnlineRecommender serves numerical features only (categorical must be empty)")
            x = x.get("numerical")
        t = x if isinstance(x, torch.Tensor) else np.asarray(x)
        if t.ndim == 1:
            t = t.reshape(1, -1)
        if t.ndim != 2 or t.shape[1] != self.input_dim:
            raise ValueError(f"expected features [nq, {self.input_dim}], got {tuple(t.shape)}")
        return t, None

    def _run(self, x: Optional[Rows], ids: Optional[np.ndarray], k: int):
        """Stage the rows, run / replay the chain, synchronise. Under ``lock``."""
        by_ids = ids is not None
        nq = len(ids) if by_ids else x.shape[0]
        if by_ids:
            self._h_ids_np[:nq] = ids
        elif isinstance(x, torch.Tensor):
            self._h_x[:nq].copy_(x)
        else:
            self._h_x_np[:nq] = x
        stream = torch.cuda.current_stream(self._d_x.device)
        key = (nq, k, by_ids)
        if os.environ.get("RTREC_ONLINE_GRAPH", "1") == "0":
            self._sequence(nq, k, by_ids)
        else:
            g = self._graphs.get(key)
            if g is not None:
                g.replay()
            else:
                # as OnlineSearcher.search: the first call at a shape answers from an
                # eager run, then the chain is captured (a capture executes nothing)
                self._sequence(nq, k, by_ids)
                stream.synchronize()
                g = torch.cuda.CUDAGraph()
                with _capture(g):
                    self._sequence(nq, k, by_ids)
                while len(self._graphs) >= self.MAX_GRAPHS:
                    self._graphs.popitem(last=False)
                self._graphs[key] = g
        stream.synchronize()
        return nq

    def _embed_any(self, x: Optional[Rows], ids: Optional[np.ndarray]) -> np.ndarray:
        """Embeddings of any number of rows; more than ``max_batch``: in chunks, copied."""
        n = len(ids) if ids is not None else x.shape[0]
        mb = self.max_batch
        if 1 <= n <= mb:
            self._run(x, ids, 0)
            return self._h_e_np[:n]
        out = np.empty((n, self.dimension), np.float32)
        for o in range(0, n, mb):
            c = min(mb, n - o)
            self._run(None if x is None else x[o:o + c], None if ids is None else ids[o:o + c], 0)
            out[o:o + c] = self._h_e_np[:c]
        return out

    # -- public --------------------------------------------------------------------
    def embed(self, user_features: Optional[Features] = None, *, user_ids=None) -> np.ndarray:
        """``[nq, d]`` fp32 unit-norm user embeddings (``get_user_embeddings`` in eval
        mode). Up to ``max_batch`` rows: a view of a pinned buffer, valid until the
        next call."""
        x, ids = self._rows_of(user_features, user_ids)
        with self.lock:
            return self._embed_any(x, ids)

    def recommend(self, user_features: Optional[Features] = None, *, user_ids=None, k: int = 10,
                  filter_ids: Optional[List[str]] = None) -> Tuple[List[List[str]], List[List[float]]]:
        """``(ids, scores)`` lists, as ``index.search(embed(...), k, filter_ids)``."""
        x, ids = self._rows_of(user_features, user_ids)
        idx = self.index
        if idx.index is None:
            raise ValueError("Index not built yet")
        nq = len(ids) if ids is not None else x.shape[0]
        k_search = min(k * 2, idx.current_size) if filter_ids else k
        if k_search <= 0 or nq == 0:
            return [[] for _ in range(nq)], [[] for _ in range(nq)]
        with self.lock:
            if k_search > OnlineSearcher.MAX_K or nq > self.max_batch:
                return idx.search(self._embed_any(x, ids), k, filter_ids)
            s = self._searcher
            if s._revalidate():  # the corpus rows moved or grew: the search graphs hold stale pointers
                for key in [key for key in self._graphs if key[1]]:
                    del self._graphs[key]
            self._run(x, ids, k_search)
            n = nq * k_search
            return _lists_from_positions(s._h_s_np[:n].reshape(nq, k_search), s._h_p_np[:n].reshape(nq, k_search),
                                         idx.id_map, k, filter_ids)
