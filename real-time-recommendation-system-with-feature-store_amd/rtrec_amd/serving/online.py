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
from .retrieval import (HipFlatIPIndex, HipIVFFlatIndex, OnlineSearcher, RetrievalEngine, _capture,
                        _exclude_positions, _lists_from_positions, _per_query)

Features = Union[np.ndarray, torch.Tensor, Dict[str, Any]]
Rows = Union[np.ndarray, torch.Tensor]


class NoDeviceError(ValueError, RuntimeError):
    """A model, table or index that is not on a ROCm device. A ``ValueError``
    like every refusal at construction, and a ``RuntimeError`` like every other
    "no CPU fallback" refusal of the package (``native.require_device``)."""


class OnlineRecommender:
    """``OnlineRecommender(model, index, max_batch=8, user_table=None)``.

    ``model``: a :class:`~rtrec_amd.models.two_tower.TwoTowerModel` (its user
    tower is served) or a tower. ``index``: a :class:`HipFlatIPIndex` or a
    :class:`HipIVFFlatIndex`, or a :class:`RetrievalEngine` whose index is one
    of them. ``user_table``: an optional
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
    Over a :class:`HipIVFFlatIndex` the searcher is the index's own
    (``index.online_searcher``: an ``OnlineIVFSearcher``, or the inner Flat
    index's searcher for a corpus that fell back to Flat) and the tail of the
    chain is its ``_device_chain``: renorm → coarse search over the centroids →
    cast → ``rt_ivf_topk`` (``rt_ivf_topk_lists`` with exclusions, in original
    positions like the seen-items CSR). ``index.nprobe`` is read at every call
    and is part of those graphs' keys. An index that switches between lists and
    the Flat fallback (``build`` / ``load``) after the recommender was made
    needs a new recommender: ``recommend`` raises ``ValueError``.
    ``RTREC_ONLINE_GRAPH=0`` (read at every call) runs the chains eagerly.

    Calls outside the graphs' range (``k_search`` > 128, more than
    ``max_batch`` rows, more than ``max_exclude`` excluded items in one call)
    embed in chunks of ``max_batch`` and call ``index.search``: the same lists,
    not resident.

    Exclusions (``recommend(exclude_items=..., exclude_seen=True)``,
    :meth:`set_seen`): the scan of the same chain reads them as CSR sources
    (``rt_flatip_topk_online_lists``) — the per-request ids through the
    searcher's two fixed-size H2D copies, the seen items from a resident CSR
    indexed by the device ids the tower gather reads. Graphs with exclusions
    are keyed ``(nq, k_search, by_ids, items, seen)``; over IVF lists every
    search graph is keyed ``(nq, k_search, by_ids, items, seen, nprobe)``.

    MMR re-rank (``recommend(mmr_lambda=..., mmr_candidates=...)``): the scan
    retrieves the candidates and ``rt_mmr_rerank`` — one more launch at the end of
    the same chain — chooses k of them; lambda travels as data, so those graphs'
    keys only gain ``("mmr", k)`` at their end and one graph serves every lambda.

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

    def __init__(self, model: nn.Module, index: Union[HipFlatIPIndex, HipIVFFlatIndex, RetrievalEngine],
                 max_batch: int = 8,
                 user_table: Optional[torch.Tensor] = None, max_exclude: int = 8192):
        if not 1 <= int(max_batch) <= self.MAX_BATCH:
            raise ValueError(f"max_batch={max_batch}: 1..{self.MAX_BATCH}")
        self.max_batch = int(max_batch)
        self.model = model
        self.tower = getattr(model, "user_tower", model)
        if isinstance(index, RetrievalEngine):
            index = index.index
        if not isinstance(index, (HipFlatIPIndex, HipIVFFlatIndex)):
            raise ValueError(f"index must be a HipFlatIPIndex or a HipIVFFlatIndex (or a RetrievalEngine over "
                             f"one), got {type(index).__name__}")
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
        if isinstance(index, HipIVFFlatIndex):
            if index.index is None:
                raise ValueError("OnlineRecommender over a HipIVFFlatIndex needs the index built: its searcher "
                                 "is sized for the lists (or for the Flat fallback of a small corpus)")
            self._searcher = index.online_searcher(mb, max_exclude)
        else:
            self._searcher = OnlineSearcher(index, mb, max_exclude)
        self.lock = self._searcher.lock
        self._seen_ids = None       # histories as given (set_seen)
        self._seen = None           # their device CSR of positions: (offsets, items)
        self._seen_generation = -1  # the index generation the CSR was mapped for
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

    def _sequence(self, nq: int, k: int, by_ids: bool, items: bool = False, seen: bool = False,
                  tags: bool = False, mmr_k: int = 0):
        """The stream-ordered chain of one call (k = 0: embed only). ``items``: the
        per-request lists staged in the searcher's pinned CSR; ``seen``: the resident
        seen-items CSR, its rows the device ids the tower gather reads; ``tags``: the
        category masks staged in the searcher's pinned mask buffer; ``mmr_k``: the k
        results of the scan are re-ranked into ``mmr_k`` (``rt_mmr_rerank``, lambda
        staged in the searcher's pinned buffer)."""
        if by_ids:
            self._d_ids[:nq].copy_(self._h_ids[:nq], non_blocking=True)
        else:
            self._d_x[:nq].copy_(self._h_x[:nq], non_blocking=True)
        self._tower(nq, by_ids)
        # the embedding leaves before the renorm rewrites the rows in place
        self._h_e[:nq].copy_(self._searcher._d_q32[:nq], non_blocking=True)
        if k:
            sources = []
            if seen:
                sources.append((self._seen[0], self._seen[1], self._d_ids))
            if items:
                self._searcher._upload_lists()
                sources.append(self._searcher._list_source())
            if tags:
                self._searcher._d_tm.copy_(self._searcher._h_tm, non_blocking=True)
            if mmr_k:
                self._searcher._d_lam.copy_(self._searcher._h_lam, non_blocking=True)
            self._searcher._device_chain(nq, k, sources, tags=tags)
            if mmr_k:
                self._searcher._device_mmr(nq, k, mmr_k)
                self._searcher._download(nq, mmr_k, True)
            else:
                self._searcher._download(nq, k)

    # -- seen items ----------------------------------------------------------------
    def set_seen(self, histories) -> None:
        """The items each user has already seen, for ``recommend(user_ids=...,
        exclude_seen=True)``: one sequence of item ids per ``user_table`` row, or a
        dict from row to sequence (other rows: nothing seen). Kept on the host as
        given and mapped to a device CSR of corpus positions (int64 offsets
        ``[n_users + 1]``, int32 positions ascending; ids the index does not know
        are ignored). Positions move on ``remove`` / ``build`` / ``load``: the CSR
        is mapped again from the kept id lists when the index generation changed;
        an in-place ``update`` moves nothing. ``None`` forgets the histories."""
        with self.lock:
            if histories is None:
                self._seen_ids = self._seen = None
            else:
                if self.user_table is None:
                    raise ValueError("set_seen needs the user_table the recommender was made with: histories "
                                     "are looked up by user_ids")
                n_users = self.user_table.shape[0]
                if isinstance(histories, dict):
                    if any(not 0 <= int(r) < n_users for r in histories):
                        raise IndexError(f"history row out of range for a table of {n_users} rows")
                elif len(histories) != n_users:
                    raise ValueError(f"{len(histories)} histories for a user_table of {n_users} rows")
                self._seen_ids = histories
                self._map_seen()
            for key in [key for key in self._graphs if len(key) > 3 and key[4]]:
                del self._graphs[key]

    def _history(self, row: int):
        h = self._seen_ids
        return h.get(row, ()) if isinstance(h, dict) else h[row]

    def _map_seen(self):
        """Kept id lists -> the device CSR of positions, for the index as it is now."""
        rev = self.index.reverse_id_map
        n_users = self.user_table.shape[0]
        offsets = np.zeros(n_users + 1, np.int64)
        parts = []
        rows = sorted(int(r) for r in self._seen_ids) if isinstance(self._seen_ids, dict) else range(n_users)
        for r in rows:
            pos = np.unique(np.asarray([rev[i] for i in self._history(r) if i in rev], dtype=np.int64))
            offsets[r + 1] = pos.size
            parts.append(pos)
        np.cumsum(offsets, out=offsets)
        flat = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
        dev = self._d_ids.device
        self._seen = (torch.from_numpy(offsets).to(dev), torch.from_numpy(flat).to(dev))
        self._seen_generation = self.index._generation

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

    def _searched(self):
        """The index the searcher has to be over: the index itself, or the inner Flat
        index of an IVF index that fell back to Flat."""
        flat = getattr(self.index, "_flat", None)
        return self.index if flat is None else flat

    def _run(self, x: Optional[Rows], ids: Optional[np.ndarray], k: int, items: bool = False, seen: bool = False,
             tags: bool = False, mmr_k: int = 0):
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
        # without exclusions the keys (and graphs) of a recommender that has none
        key = (nq, k, by_ids, items, seen) if (items or seen) else (nq, k, by_ids)
        nprobe = getattr(self._searcher, "_nprobe", 0)   # OnlineIVFSearcher: read from the index at this call
        if k and nprobe:
            key = (nq, k, by_ids, items, seen, nprobe)
        seq = (nq, k, by_ids, items, seen, tags, mmr_k)
        if tags:   # one more flag, at the end: one graph serves every mask value
            key = (nq, k, by_ids, items, seen) + key[5:] + ("tags",)
        if mmr_k:  # at the very end, lambda being data: one graph serves every value
            key = key + ("mmr", mmr_k)
        if os.environ.get("RTREC_ONLINE_GRAPH", "1") == "0":
            self._sequence(*seq)
        else:
            g = self._graphs.get(key)
            if g is not None:
                g.replay()
            else:
                # as OnlineSearcher.search: the first call at a shape answers from an
                # eager run, then the chain is captured (a capture executes nothing)
                self._sequence(*seq)
                stream.synchronize()
                g = torch.cuda.CUDAGraph()
                with _capture(g):
                    self._sequence(*seq)
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
                  filter_ids: Optional[List[str]] = None, exclude_items=None, exclude_seen: bool = False,
                  filter_categories=None, exclude_categories=None,
                  mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None
                  ) -> Tuple[List[List[str]], List[List[float]]]:
        """``(ids, scores)`` lists, as ``index.search(embed(...), k, filter_ids)``.

        ``exclude_items`` (the request schema's field, src/api/schemas.py:31-34):
        item ids not to return, as ``exclude_ids`` of ``HipFlatIPIndex.search`` —
        one list for every row or one per row, unknown ids ignored, exact.
        ``exclude_seen``: also leave out what :meth:`set_seen` recorded for each of
        ``user_ids`` (the evaluator's train-item mask, src/evaluation/metrics.py:
        252-282); the scan reads the resident CSR through the device ids of the
        tower gather, so a request uploads no history. Both may be given: two
        sources of one scan. ``ValueError`` without ``user_ids`` or before
        ``set_seen``.
        ``filter_categories`` / ``exclude_categories`` (the request schema's
        ``filter_categories``): as ``HipFlatIPIndex.search`` — tested by the same
        scan, composing with both exclusion sources; one more fixed-size H2D copy
        in the chain, one graph for every mask value.
        ``mmr_lambda`` / ``mmr_candidates``: as ``HipFlatIPIndex.search`` — the
        ranking stage of the request path (src/serving/service.py:204-228): the top
        ``mmr_candidates`` (default ``min(10 * k, 128, index size)``) are re-ranked
        into k by ``rt_mmr_rerank``, one more launch at the end of the same chain;
        lambda is data (one fixed-size H2D copy), so the graph key gains only
        ``("mmr", k)`` and one graph serves every lambda. Not with ``filter_ids``."""
        x, ids = self._rows_of(user_features, user_ids)
        idx = self.index
        n_cand = idx._mmr_args(k, mmr_lambda, mmr_candidates, filter_ids)
        if idx.index is None:
            raise ValueError("Index not built yet")
        if exclude_seen and ids is None:
            raise ValueError("exclude_seen looks histories up by user_ids")
        if exclude_seen and self._seen_ids is None:
            raise ValueError("exclude_seen needs set_seen(histories) first")
        nq = len(ids) if ids is not None else x.shape[0]
        k_search = n_cand if n_cand else (min(k * 2, idx.current_size) if filter_ids else k)
        if k_search <= 0 or nq == 0:
            return [[] for _ in range(nq)], [[] for _ in range(nq)]
        items = exclude_items is not None
        masks = idx._query_masks(filter_categories, exclude_categories, nq)
        cats = {} if masks is None else dict(filter_categories=filter_categories,
                                             exclude_categories=exclude_categories)
        if n_cand:
            cats.update(mmr_lambda=mmr_lambda, mmr_candidates=n_cand)
        with self.lock:
            s = self._searcher
            resident = k_search <= OnlineSearcher.MAX_K and nq <= self.max_batch
            if resident and items:
                resident = s._stage_lists(nq, _exclude_positions(idx.reverse_id_map, exclude_items, nq))
            if not resident:
                excl = None
                if items or exclude_seen:  # per row: the request's ids and the row's history
                    excl = [list(e) for e in _per_query(exclude_items, nq)] if items else [[] for _ in range(nq)]
                    if exclude_seen:
                        for q, u in enumerate(ids):
                            excl[q].extend(self._history(int(u)))
                return idx.search(self._embed_any(x, ids), k, filter_ids, exclude_ids=excl, **cats)
            if s.index is not self._searched():
                raise ValueError("the index switched between its lists and the Flat fallback (or was rebuilt "
                                 "onto another inner index) since this recommender was made: make a new one")
            if s._revalidate():  # the corpus rows moved or grew: the search graphs hold stale pointers
                for key in [key for key in self._graphs if key[1]]:
                    del self._graphs[key]
            if exclude_seen and self._seen_generation != idx._generation:
                self._map_seen()  # positions moved (remove / build / load): new tensors, no graph holds the old
                for key in [key for key in self._graphs if len(key) > 3 and key[4]]:
                    del self._graphs[key]
            if masks is not None:
                s._stage_tags(nq, masks)
            if n_cand:
                s._stage_mmr(nq, mmr_lambda)
            self._run(x, ids, k_search, items, exclude_seen, tags=masks is not None, mmr_k=k if n_cand else 0)
            k_got = k if n_cand else k_search
            n = nq * k_got
            return _lists_from_positions(s._h_s_np[:n].reshape(nq, k_got), s._h_p_np[:n].reshape(nq, k_got),
                                         idx.id_map, k, filter_ids)
