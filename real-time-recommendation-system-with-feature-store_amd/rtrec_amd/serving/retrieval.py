"""Retrieval layer: the reference's ``IndexBase`` / ``RetrievalEngine`` surface
(src/serving/retrieval.py:16-46, 505-692) over an MI355X-resident exact
inner-product index.

``HipFlatIPIndex`` is the drop-in for ``FaissIndex`` in ``Flat`` mode
(retrieval.py:49-329): same constructor config keys, same
``build/search/add/save/load`` behaviour and errors, same ``(ids, scores)``
result lists, but the corpus lives in HBM and ``search`` runs the gfx950
Flat-IP top-K kernel (MFMA scoring + wavefront select) instead of Faiss-CPU.
"""
from __future__ import annotations

import contextlib
import gc
import hashlib
import json
import os
import pickle
import struct
import threading
import time
from collections import OrderedDict
from abc import ABC, abstractmethod
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import kernels

Array = Union[np.ndarray, torch.Tensor]


class _Log:
    """Tiny stand-in for the reference's loguru calls (loguru is not a dependency)."""

    def __init__(self):
        import logging
        self._l = logging.getLogger("rtrec_amd.retrieval")

    def info(self, *a):
        self._l.info(*a)

    def warning(self, *a):
        self._l.warning(*a)

    def debug(self, *a):
        self._l.debug(*a)


logger = _Log()


class IndexBase(ABC):
    """Abstract base class for ANN indices (retrieval.py:16-46)."""

    @abstractmethod
    def build(self, embeddings: np.ndarray, ids: List[str]):
        """Build the index from embeddings."""

    @abstractmethod
    def search(self, query_embeddings: np.ndarray, k: int = 10) -> Tuple[np.ndarray, np.ndarray]:
        """Search for nearest neighbors."""

    @abstractmethod
    def add(self, embeddings: np.ndarray, ids: List[str]):
        """Add new embeddings to the index."""

    @abstractmethod
    def save(self, path: str):
        """Save index to disk."""

    @abstractmethod
    def load(self, path: str):
        """Load index from disk."""


_STORAGE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


MAX_DIM = 256   # rt_flatip_topk: d <= 256 (f32 d % 4 == 0, f16/bf16 d % 8 == 0)
MAX_K_L2 = 512  # IndexFlatL2 mode: k <= 512 (its exact re-selection holds k_sel <= 512 candidates);
                # the inner-product modes take any k (kernels.flatip_topk: k > 512 in exact 512-wide passes)


def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("HipFlatIPIndex needs a ROCm device (no CPU fallback in the MI355X build)")
    return torch.device("cuda", torch.cuda.current_device())


class _HbmIndex(IndexBase):
    """What the HBM-resident indexes share: the common config keys and their
    validation, the device, the preparation of rows and queries, the id
    bookkeeping and its ``.pkl`` payload, and — for the two single-GPU indexes —
    the front of ``search``."""

    # whether the resident searcher takes ``exclude`` lists (it reads them in its
    # scan); otherwise a call with ``exclude_ids`` goes to the bitmap path
    _searcher_takes_exclude = False

    def __init__(self, config: Dict[str, Any]):
        self.config = config
        self.dimension = config.get("dimension", 128)
        self.metric = config.get("metric", "cosine")
        # retrieval.py:96-100: "cosine" → IndexFlatIP on normalised rows, any other
        # metric → IndexFlatL2; "inner_product" (this build's extension) → raw IP
        self._l2 = self.metric not in ("cosine", "inner_product")
        self.storage_dtype = _STORAGE[config.get("storage_dtype", "float32")]
        self._check_metric()
        # what rt_flatip_topk serves (include/rtrec_hip.h): fail at construction,
        # not at the first search
        d_max = MAX_DIM - 4 if self._l2 else MAX_DIM
        step = 4 if self.storage_dtype == torch.float32 else 8
        if not (0 < self.dimension <= d_max) or self.dimension % step:
            raise ValueError(f"dimension {self.dimension} unsupported: the MI355X index serves d % {step} == 0, "
                             f"d <= {d_max}" + self._dimension_detail())
        dev = config.get("device")
        self.device = torch.device(dev) if dev is not None else None
        self._reset_ids()
        self.current_size = 0
        self._generation = 0   # bumped by build / add / load / remove (OnlineSearcher validity)
        self._init_categories()

    def _check_metric(self):
        """Raise for a metric (or a metric / storage pair) the class does not serve."""

    # -- categories (the request schema's filter_categories, src/api/schemas.py:21-34) --
    MAX_CATEGORIES = 64

    def _init_categories(self):
        """The ``categories`` option: the vocabulary (at most 64 names; category j is
        bit j of an item's tags), or absent — the feature is off."""
        names = self.config.get("categories")
        self.categories: Optional[List[str]] = None if names is None else [str(c) for c in names]
        # [capacity] int64 on the device, by position; the first current_size are valid.
        # It moves (a new tensor) only where the generation is bumped too.
        self._tags: Optional[torch.Tensor] = None
        self._cat_bit: Dict[str, int] = {}
        if self.categories is None:
            return
        if len(self.categories) > self.MAX_CATEGORIES or len(set(self.categories)) != len(self.categories):
            raise ValueError(f"categories: at most {self.MAX_CATEGORIES} distinct names, got {len(self.categories)}")
        self._check_categories()
        self._cat_bit = {c: j for j, c in enumerate(self.categories)}

    def _check_categories(self):
        """Raise where the class (or its mode) does not serve category filters."""
        if self._l2:
            raise ValueError("categories: the filters are served for the inner-product metrics ('cosine', "
                             "'inner_product'), not in the L2 mode")

    def _need_categories(self, keyword: str):
        if self.categories is None:
            raise ValueError(f"{keyword}: this index has no category vocabulary — set the config key 'categories' "
                             "(a list of at most 64 names)")

    def _mask_of(self, names) -> int:
        m = 0
        for c in names:
            bit = self._cat_bit.get(c)
            if bit is None:
                raise ValueError(f"unknown category {c!r} (config key 'categories': {self.categories})")
            m |= 1 << bit
        return m

    def _item_tags(self, item_categories, n: int) -> np.ndarray:
        """``item_categories`` of ``n`` items as uint64 masks: None = untagged; an
        integer array of masks; or per item a sequence of category names."""
        if item_categories is None:
            return np.zeros(n, np.uint64)
        self._need_categories("item_categories")
        if isinstance(item_categories, torch.Tensor):
            item_categories = item_categories.cpu().numpy()
        if isinstance(item_categories, np.ndarray) and item_categories.dtype.kind in "iu":
            masks = item_categories.reshape(-1).astype(np.int64, copy=False).view(np.uint64) \
                if item_categories.dtype.kind == "i" else item_categories.reshape(-1).astype(np.uint64)
        else:
            item_categories = list(item_categories)
            if item_categories and all(isinstance(c, (int, np.integer)) for c in item_categories):
                masks = np.array([int(c) & 0xFFFFFFFFFFFFFFFF for c in item_categories], dtype=np.uint64)
            else:
                masks = np.array([self._mask_of([c] if isinstance(c, str) else c) for c in item_categories],
                                 dtype=np.uint64).reshape(-1)
        if masks.shape[0] != n:
            raise ValueError(f"item_categories holds {masks.shape[0]} entries for {n} items")
        if len(self.categories) < 64 and masks.size and int(masks.max()) >> len(self.categories):
            raise ValueError(f"item_categories: a mask has bits past the {len(self.categories)} categories")
        return masks

    def _query_masks(self, filter_categories, exclude_categories, nq: int):
        """(any_of, none_of) uint64 [nq] of a search's ``filter_categories`` /
        ``exclude_categories`` — one list of names for all queries, or one list per
        query — or None when neither is given."""
        if filter_categories is None and exclude_categories is None:
            return None
        self._need_categories("filter_categories" if filter_categories is not None else "exclude_categories")
        out = []
        for names in (filter_categories, exclude_categories):
            if names is None:
                out.append(np.zeros(nq, np.uint64))
                continue
            if isinstance(names, str):
                names = [names]
            out.append(np.array([self._mask_of(per) for per in _per_query(names, nq)], dtype=np.uint64))
        return out[0], out[1]

    def _tags_store(self, start: int, masks: np.ndarray):
        """Tags of the positions [start, start + len(masks)); grows like the rows."""
        if self.categories is None:
            return
        n_new = start + len(masks)
        if self._tags is None or self._tags.numel() < n_new:
            cap = max(n_new, 2 * (self._tags.numel() if self._tags is not None else 0), 1024)
            buf = torch.zeros(cap, dtype=torch.int64, device=self._dev())
            if self._tags is not None and start:
                buf[:start].copy_(self._tags[:start])
            self._tags = buf
        if len(masks):
            self._tags[start:n_new].copy_(torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)))

    def _tags_write(self, positions: List[int], masks: np.ndarray):
        """In place, by position: no pointer changes, captured graphs stay valid."""
        if not len(positions):
            return
        dev = self._dev()
        pos = torch.tensor(list(positions), dtype=torch.int64, device=dev)
        with self._searcher_lock():
            self._tags[pos] = torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)).to(dev)

    def set_item_categories(self, ids: List[str], item_categories):
        """Replace the categories of known items (``item_categories`` as ``build``
        takes it; None = untagged), in place in the resident tags tensor: no
        generation bump, resident searchers keep their captured graphs and read
        the new tags at their next replay. An unknown id raises."""
        self._need_categories("set_item_categories")
        if self._tags is None:
            raise ValueError("Index not built yet")
        ids = list(ids)
        missing = [i for i in ids if i not in self.reverse_id_map]
        if missing:
            raise ValueError(f"set_item_categories: unknown ids {missing[:5]}")
        self._tags_write([self.reverse_id_map[i] for i in ids], self._item_tags(item_categories, len(ids)))

    def item_tags(self) -> np.ndarray:
        """uint64 [current_size]: the tags by position."""
        if self._tags is None:
            return np.zeros(self.current_size, np.uint64)
        return self._tags[: self.current_size].cpu().numpy().view(np.uint64)

    def _tags_path(self, path: Path) -> Path:
        return path.with_suffix(".tags.npz")

    def _save_tags(self, path: Path):
        """``<path>.tags.npz``: vocabulary and tags, beside the other files."""
        f = self._tags_path(path)
        if self.categories is None:
            if f.exists():
                f.unlink()   # a stale file of an earlier save under this name
            return
        np.savez(f, categories=np.array(self.categories, dtype=str), tags=self.item_tags())

    def _load_tags(self, path: Path):
        """After the rows and the config were loaded: the vocabulary (the file's, when
        there is one) and the tags of the ``current_size`` positions."""
        f = self._tags_path(path)
        self._init_categories()
        if not f.exists():
            if self.categories is not None:
                self._tags_store(0, np.zeros(self.current_size, np.uint64))
            return
        with np.load(f) as z:
            self.categories = [str(c) for c in z["categories"]]
            tags = z["tags"].astype(np.uint64)
        self.config = dict(self.config, categories=list(self.categories))
        self._cat_bit = {c: j for j, c in enumerate(self.categories)}
        self._tags = None
        self._tags_store(0, tags[: self.current_size])

    def _dimension_detail(self) -> str:
        """The class's own tail of the dimension error."""
        return ""

    def _init_online(self):
        """The ``online_max_batch`` option of the indexes that hold a resident searcher."""
        self.online_max_batch = int(self.config.get("online_max_batch", 0) or 0)
        if not 0 <= self.online_max_batch <= OnlineSearcher.MAX_BATCH:
            raise ValueError(f"online_max_batch={self.online_max_batch}: 0 (off) or 1..{OnlineSearcher.MAX_BATCH}")
        self._online: Optional["OnlineSearcher"] = None

    # -- device, rows ------------------------------------------------------
    def _dev(self) -> torch.device:
        if self.device is None:
            self.device = _default_device()
        return self.device

    def _renorm_(self, t: torch.Tensor) -> torch.Tensor:
        return kernels.l2_renorm_(t)

    def _prepare(self, x: Array) -> torch.Tensor:
        """Copy to a contiguous fp32 device tensor (the index owns its vectors,
        retrieval.py:82) and renormalise in place for the cosine metric
        (retrieval.py:86)."""
        t = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x
        if t.dim() == 1:
            t = t.reshape(1, -1)
        t = t.to(device=self._dev(), dtype=torch.float32, copy=True).contiguous()
        if t.shape[1] != self.dimension:
            raise ValueError(f"expected dimension {self.dimension}, got {t.shape[1]}")
        if self.metric == "cosine" and t.shape[0]:
            self._renorm_(t)
        return t

    def _searcher_lock(self):
        """The resident searcher's lock when the index holds one: its replays read the rows."""
        return self._online.lock if self._online is not None else contextlib.nullcontext()

    # -- ids ---------------------------------------------------------------
    def _reset_ids(self):
        self.id_map: Dict[int, str] = {}
        self.reverse_id_map: Dict[str, int] = {}
        self._ids: List[Optional[str]] = []        # position -> id (vectorised id_map)

    def _record_ids(self, start: int, ids: List[str], n_rows: int):
        """Name the ``n_rows`` rows appended at position ``start``: both maps take
        every id given, ``_ids`` one entry per row (None past the ids)."""
        for i, item_id in enumerate(ids):
            self.id_map[start + i] = item_id
            self.reverse_id_map[item_id] = start + i
        self._ids.extend(list(ids)[:n_rows] + [None] * max(0, n_rows - len(ids)))

    def _save_ids(self, path: Path, **extra):
        """``<path>.pkl``: the id maps, the size and the config (the reference's keys)."""
        with open(path.with_suffix(".pkl"), "wb") as f:
            pickle.dump({"id_map": self.id_map, "reverse_id_map": self.reverse_id_map,
                         "current_size": self.current_size, "config": self.config, **extra}, f)

    @staticmethod
    def _read_pkl(path: Path) -> Dict[str, Any]:
        with open(path.with_suffix(".pkl"), "rb") as f:
            return pickle.load(f)  # files this package wrote (same layout as the reference's)

    def _load_ids(self, data: Dict[str, Any], n: int):
        """The id maps of a ``.pkl`` payload over ``n`` rows."""
        self.id_map = data["id_map"]
        self.reverse_id_map = data["reverse_id_map"]
        self._ids = [self.id_map.get(i) for i in range(n)]

    # -- MMR re-ranking (the ranking stage of the request path, src/serving/service.py:204-228) --
    MMR_MAX_CANDIDATES = kernels.MMR_MAX_CAND

    def _check_mmr(self):
        """Raise where the class (or its mode) does not serve the MMR re-rank."""
        if self._l2:
            raise ValueError("mmr_lambda: the MMR re-rank is served for the inner-product metrics ('cosine', "
                             "'inner_product'), not in the L2 mode")

    def _mmr_args(self, k: int, mmr_lambda: Optional[float], mmr_candidates: Optional[int],
                  filter_ids=None) -> Optional[int]:
        """The candidates per query of a re-ranked search (None: ``mmr_lambda`` is None,
        the re-rank is off). The default is the reference's 10x over-fetch
        (service.py:206) clamped to the kernel's cap and to the corpus:
        ``min(10 * k, 128, current_size)``, and never below ``min(k, 128)``."""
        if mmr_lambda is None:
            if mmr_candidates is not None:
                raise ValueError("mmr_candidates without mmr_lambda: the re-rank is off (mmr_lambda=None)")
            return None
        self._check_mmr()
        if not 0.0 <= float(mmr_lambda) <= 1.0:   # a NaN fails too
            raise ValueError(f"mmr_lambda={mmr_lambda}: 0 <= mmr_lambda <= 1")
        if filter_ids is not None:
            raise ValueError("filter_ids together with mmr_lambda: the allow-list is a host post-filter over a 2k "
                             "over-fetch; combining it with the re-rank is out of scope")
        cap = self.MMR_MAX_CANDIDATES
        if mmr_candidates is None:
            mmr_candidates = max(min(10 * k, cap, self.current_size), min(k, cap))
        if not k <= int(mmr_candidates) <= cap:
            raise ValueError(f"mmr_candidates={mmr_candidates}: k <= mmr_candidates <= {cap} (k={k})")
        return int(mmr_candidates)

    def _mmr_operands(self) -> Tuple[torch.Tensor, Optional[torch.Tensor], int]:
        """(rows, pos_slot, n_pos) of ``kernels.mmr_rerank`` over this index: the stored
        rows, the stored row of a position (None: the identity) and the number of positions."""
        raise NotImplementedError

    def mmr_rerank_tensors(self, scores: torch.Tensor, positions: torch.Tensor, k: int, mmr_lambda
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Re-rank what ``search_tensors`` returned — (scores, positions) ``[nq, n_cand]``
        on the device, n_cand <= 128 — into the MMR choice of ``k`` per query
        (``rt_mmr_rerank`` over the index's own stored rows; similarities are cosines
        unless the metric is ``"cosine"``, whose rows are stored unit-norm): device
        (scores, positions) ``[nq, k]`` in selection order, original scores."""
        self._check_mmr()
        rows, pos_slot, n_pos = self._mmr_operands()
        return kernels.mmr_rerank(scores.contiguous(), positions.contiguous(), rows, k, mmr_lambda, pos_slot=pos_slot,
                                  n_pos=n_pos, normalize=self.metric != "cosine")

    # -- search (the single-GPU indexes) -------------------------------------
    def search(self, query_embeddings: Array, k: int = 10, filter_ids: Optional[List[str]] = None,
               exclude_ids=None, filter_categories=None, exclude_categories=None,
               mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None
               ) -> Tuple[List[List[str]], List[List[float]]]:
        """retrieval.py:141-197: normalise, top-k_search (2k when filtering), map
        positions to ids, drop -1 padding, apply the filter, stop at k.

        ``exclude_ids`` (the request schema's ``exclude_items``, src/api/schemas.py:
        31-34): item ids that must not be returned — one list for every query, or
        one list per query; unknown ids are ignored. Unlike ``filter_ids`` the
        exclusion is applied IN the search and is exact: k results whenever k
        eligible items exist, in every configuration (a resident searcher that
        takes lists reads them in its scan; the other paths mask through a
        bitmap). With ``filter_ids`` as well, the allow-list then applies to the
        2k over-fetch.

        ``filter_categories`` / ``exclude_categories`` (the request schema's
        ``filter_categories``; config key ``categories``): names of the vocabulary —
        one list for every query, or one list per query; an unknown name raises.
        An item is eligible iff it carries at least one of ``filter_categories``
        (when given and not empty) and none of ``exclude_categories``. Like
        ``exclude_ids`` the filter is applied IN the search and is exact over the
        rows scanned (for an IVF index: the probed lists, as with Faiss), and it
        composes with ``exclude_ids`` by union of what is skipped. Calls within
        the online limits stay on the resident searcher (the scan tests the tags
        itself); the others go through ``rt_tag_filter_bitmap``.

        ``mmr_lambda`` (None = off; 0 <= mmr_lambda <= 1) / ``mmr_candidates``
        (default ``min(10 * k, 128, current_size)``; k <= mmr_candidates <= 128):
        the ranking stage of the request path (src/serving/service.py:204-228) as
        Maximal Marginal Relevance — the top ``mmr_candidates`` are retrieved as
        above, exclusions and category filters included, and ``rt_mmr_rerank``
        chooses k of them greedily by ``mmr_lambda * score - (1 - mmr_lambda) * max
        similarity to what is already chosen`` over the index's own stored rows
        (similarities are cosines). The lists come in selection order with the
        original scores, so they are no longer score-sorted. Calls within the
        online limits stay resident (one more launch in the captured chain, lambda
        is data: one graph serves every value); the others re-rank the device
        tensors of ``search_tensors`` and copy k results per query to the host.
        Not with ``filter_ids``, not in the L2 mode: ``ValueError``."""
        n_cand = self._mmr_args(k, mmr_lambda, mmr_candidates, filter_ids)
        if self.index is None:
            raise ValueError("Index not built yet")
        k_search = n_cand if n_cand else (min(k * 2, self.current_size) if filter_ids else k)
        nq = 1 if np.ndim(query_embeddings) == 1 else len(query_embeddings)
        if k_search <= 0 or (self.mutable and self.current_size == 0):  # emptied by remove: nothing to scan
            return [[] for _ in range(nq)], [[] for _ in range(nq)]
        excl = None if exclude_ids is None else _exclude_positions(self.reverse_id_map, exclude_ids, nq)
        masks = self._query_masks(filter_categories, exclude_categories, nq)
        if self.online_max_batch and not self._l2 and k_search <= OnlineSearcher.MAX_K \
                and 1 <= nq <= self.online_max_batch and (excl is None or self._searcher_takes_exclude):
            if self._online is None:
                self._online = self.online_searcher(self.online_max_batch)
            with self._online.lock:  # the returned buffers are the searcher's: read them under its lock
                if n_cand:
                    scores, pos = self._online.search(query_embeddings, k_search, exclude=excl, tags=masks,
                                                      mmr=(k, mmr_lambda))
                else:
                    scores, pos = self._online.search(query_embeddings, k_search, exclude=excl, tags=masks)
                return _lists_from_positions(scores, pos, self.id_map, k, filter_ids)
        bits = None if excl is None else kernels.exclusion_bitmap(nq, self.current_size, excl, self._dev())
        scores, pos = self.search_tensors(query_embeddings, k_search, exclude_bits=bits, tag_filter=masks)
        if n_cand:
            scores, pos = self.mmr_rerank_tensors(scores, pos, k, mmr_lambda)
        return _lists_from_positions(scores.cpu().numpy(), pos.cpu().numpy(), self.id_map, k, filter_ids)

    def _filter_bits(self, tag_filter, nq: int, exclude_bits: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """``search_tensors``' ``tag_filter=(any_of, none_of)`` (uint64 / int64 masks
        ``[nq]``, numpy or tensors; either may be None) as an exclusion bitmap:
        ``rt_tag_filter_bitmap`` over the resident tags, accumulated onto
        ``exclude_bits`` (a copy) when the call has one."""
        if tag_filter is None:
            return exclude_bits
        self._need_categories("tag_filter")
        if len(tag_filter) != 2:
            raise ValueError("tag_filter is (any_of, none_of)")
        any_of, none_of = (_mask_tensor(m, nq, self._dev()) for m in tag_filter)
        n = self.current_size
        words = (n + 31) // 32
        out = None
        if exclude_bits is not None:
            if exclude_bits.shape[0] != nq or exclude_bits.shape[1] < words:
                raise ValueError("exclude_bits has fewer words than ceil(n_items / 32)")
            out = exclude_bits.contiguous().clone()
        return kernels.tag_filter_bitmap(self._tags, any_of, none_of, nq, n_items=n, out=out,
                                         accumulate=out is not None)


class HipFlatIPIndex(_HbmIndex):
    """Exact inner-product index resident in HBM (FaissIndex ``Flat`` semantics).

    Config keys (retrieval.py:58-63): ``dimension`` (128), ``metric``
    ("cosine" → normalize_L2 on build/add/search + inner product, like
    IndexFlatIP; any other value → squared L2 distances ascending, like
    IndexFlatL2, float32 rows; "inner_product" → raw inner product, this
    build's extension),
    ``index_factory`` (only recorded: every factory is served exactly),
    ``nprobe`` (ignored, exact), plus ``device`` and ``storage_dtype``
    ("float32" default = Faiss numerics; "float16"/"bfloat16" halve the bytes).

    ``online_max_batch`` (default 0 = off; 1..8): ``search`` calls with at most
    that many queries and ``k_search`` <= 128 (``k_search`` = 2k with
    ``filter_ids``) go through a resident :class:`OnlineSearcher` — pinned
    buffers, one graph replay, one synchronise, the row-streaming
    ``rt_flatip_topk_online`` kernel pair — and return the same lists as the
    default path. It is meant for the per-request shape of the serving path
    (src/serving/service.py:268-302: one user embedding per call). Measured
    ("Online search"): recommended for every call it serves —
    p50 of ``search`` 10-13 % lower at N = 1,000, d = 128, k = 50 fp32 (where
    launch-plus-synchronise latency is the floor), 3-13x lower at N = 10^6,
    d = 128, k = 100, float16 and float32, nq = 1 and 8.
    Larger calls take the default path. Inner-product metrics only: with the L2
    metric the option raises ``ValueError``.

    ``mutable`` (default False: ``update`` and ``remove`` only warn, like the
    reference's Flat index, retrieval.py:228-246). With it on, ``update`` is an
    upsert — a known id's row is overwritten in place (``rt_scatter_rows``; no
    pointer or size changes, so resident searchers keep their captured graphs
    and see the new row at their next replay), an unknown id is appended
    through ``add`` — and ``remove`` compacts the corpus in row order
    (``rt_rows_compact``), as ``faiss.IndexFlat.remove_ids`` does: later rows
    shift down, the corpus stays dense, and the index is indistinguishable
    from one built on the surviving rows (stored bits, positions, the
    lower-position-wins tie rule). Every metric and storage dtype.

    ``categories`` (default absent = off): the vocabulary of the category
    filters, at most 64 names (inner-product metrics). ``build`` / ``add`` /
    ``update`` then take ``item_categories`` (per item a sequence of names, or
    uint64 masks: an item belongs to several categories at once),
    ``set_item_categories`` rewrites tags in place, and ``search`` takes
    ``filter_categories`` / ``exclude_categories``: exact, applied by the scan
    itself on the resident path (``rt_flatip_topk_online_tags``), through
    ``rt_tag_filter_bitmap`` elsewhere; ``save`` adds ``<path>.tags.npz``.
    Measured ("Category filters"; 1M x 128, k = 100, nq 1 and 8, float16 and
    float32, 50 / 10 / 1 % of the items eligible; p50 of the resident call in us): 95-215
    without a filter, 95-212 with it (-28 to 11 us), against 922-3536 through the bitmap route.

    ``search(..., mmr_lambda=, mmr_candidates=)`` (default off): the ranking stage of
    the request path (src/serving/service.py:204-228) as an MMR re-rank of the top
    ``mmr_candidates`` into k over the stored rows (``rt_mmr_rerank``); resident
    within the online limits (one more launch in the chain, lambda as data), on the
    device tensors of ``search_tensors`` otherwise (``mmr_rerank_tensors``).
    Inner-product metrics, not with ``filter_ids`` ("MMR re-ranking").
    """

    _searcher_takes_exclude = True   # OnlineSearcher: rt_flatip_topk_online_lists

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config or {})
        self.index_factory = self.config.get("index_factory", "Flat")
        self.nprobe = self.config.get("nprobe", 20)
        self.index: Optional[torch.Tensor] = None   # [capacity, d] device rows; first current_size valid
        self.mutable = bool(self.config.get("mutable", False))
        self._init_online()
        if self.online_max_batch and self._l2:
            raise ValueError("online_max_batch serves the inner-product metrics ('cosine', 'inner_product'); "
                             "the L2 metric keeps the default search path")
        if "IVF" in str(self.index_factory):
            logger.warning("index_factory %s: the MI355X index serves every factory exactly (Flat)",
                           self.index_factory)

    def _check_metric(self):
        if self._l2 and self.storage_dtype != torch.float32:
            raise ValueError("the L2 metric (IndexFlatL2) stores float32 rows, like Faiss")

    def _dimension_detail(self) -> str:
        return f" for {self.metric!r} / {self.config.get('storage_dtype', 'float32')}"

    # -- helpers -----------------------------------------------------------
    def _row_width(self) -> int:
        """Stored row width: d, or d + 4 augmented columns in the L2 mode
        ([x, -||x||^2/2, 0, 0, 0], rt_l2_augment_f32)."""
        return self.dimension + 4 if self._l2 else self.dimension

    def _to_storage(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Prepared rows -> the rows as stored ([n, _row_width()] storage dtype):
        the dtype cast, and ``l2_augment`` in the L2 mode. Per row, so a row's
        stored bits do not depend on what it is stored with."""
        rows = rows.to(self.storage_dtype)
        if self._l2:
            return kernels.l2_augment(rows, 1, out=out)
        if out is None:
            return rows
        out.copy_(rows)
        return out

    def _store(self, rows: torch.Tensor):
        n_new = self.current_size + rows.shape[0]
        if self.index is None or self.index.shape[0] < n_new:
            cap = max(n_new, 2 * (self.index.shape[0] if self.index is not None else 0), 1024)
            buf = torch.empty((cap, self._row_width()), dtype=self.storage_dtype, device=self._dev())
            if self.index is not None and self.current_size:
                buf[: self.current_size].copy_(self.index[: self.current_size])
            self.index = buf
        self._to_storage(rows, out=self.index[self.current_size:n_new])

    # -- IndexBase ---------------------------------------------------------
    def build(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:70-139 (Flat path). ``item_categories`` (config key
        ``categories``): per item a sequence of category names, or an integer
        array of 64-bit masks; None = untagged."""
        start = time.time()
        rows = self._prepare(embeddings)
        tags = self._item_tags(item_categories, rows.shape[0])
        self.index = None
        self.current_size = 0
        self._reset_ids()
        self._store(rows)
        self._tags = None
        self._tags_store(0, tags)
        self._record_ids(0, ids, max(rows.shape[0], len(ids)))   # ids past the rows stay in _ids
        self.current_size = rows.shape[0]
        self._generation += 1
        self._online = None  # sized for the index as it was; the next small call makes a new one
        logger.info("Index built in %.2f seconds", time.time() - start)

    def online_searcher(self, max_batch: int = 8, max_exclude: int = 8192) -> "OnlineSearcher":
        """A resident searcher for calls of at most ``max_batch`` (1..8) queries
        and k <= 128 over this index (inner-product metrics); ``max_exclude``:
        the exclusion-list entries one call may carry through its resident buffers."""
        return OnlineSearcher(self, max_batch, max_exclude)

    def search_tensors(self, query_embeddings: Array, k: int,
                       exclude_bits: Optional[torch.Tensor] = None, tag_filter=None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-level search: (scores [nq,k], positions [nq,k]) with -1 padding;
        scores are inner products (descending) or, in the L2 mode, squared L2
        distances (ascending, IndexFlatL2.search). ``tag_filter=(any_of, none_of)``:
        per-query 64-bit category masks; the ineligible items join ``exclude_bits``
        through ``rt_tag_filter_bitmap``."""
        if self.index is None:
            raise ValueError("Index not built yet")
        q = self._prepare(query_embeddings).to(self.storage_dtype)
        exclude_bits = self._filter_bits(tag_filter, q.shape[0], exclude_bits)
        if self._l2:
            if k > MAX_K_L2:
                raise ValueError(f"k={k} > {MAX_K_L2}: the MI355X IndexFlatL2 mode returns at most {MAX_K_L2} "
                                 "results per query (the inner-product metrics take any k)")
            return kernels.flatl2_topk(kernels.l2_augment(q, 0), self.index[: self.current_size], self.dimension, k,
                                       exclude_bits=exclude_bits)
        return kernels.flatip_topk(q, self.index[: self.current_size], k, exclude_bits=exclude_bits)

    def _mmr_operands(self):
        return self.index[: self.current_size], None, self.current_size   # position p is stored row p

    def add(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:199-226: incremental append (Kafka item_update path);
        ``item_categories`` as ``build`` takes it."""
        if self.index is None:
            raise ValueError("Index not built yet")
        rows = self._prepare(embeddings)
        self._append(rows, ids, self._item_tags(item_categories, rows.shape[0]))

    def _append(self, rows: torch.Tensor, ids: List[str], tags: Optional[np.ndarray] = None):
        """Append prepared rows, their ids and tags (``add``; the unknown ids of ``update``)."""
        self._store(rows)
        self._tags_store(self.current_size, np.zeros(rows.shape[0], np.uint64) if tags is None else tags)
        self._record_ids(self.current_size, ids, max(rows.shape[0], len(ids)))
        self.current_size += rows.shape[0]
        self._generation += 1
        logger.info("Added %d items to index. Total size: %d", rows.shape[0], self.current_size)

    def update(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:228-237: a no-op with a warning, like the reference, unless
        the index is ``mutable``. ``item_categories``: as ``build`` takes it; None
        keeps the tags of known ids (unknown ids are appended untagged); given,
        a known id's tags are overwritten in place like its row.
        Then an upsert: rows are prepared and stored as
        ``build`` would store them; a known id's row is overwritten in place (the
        last occurrence of an id given more than once wins; an id stored twice
        through ``add`` has its last row overwritten, the one ``reverse_id_map``
        names) without a generation bump — no pointer or size changes, captured
        graphs of resident searchers stay valid; unknown ids are appended as by
        ``add``, in call order."""
        if not self.mutable:
            logger.warning("Flat index doesn't support direct updates. Consider periodic rebuilds.")
            return
        if self.index is None:
            raise ValueError("Index not built yet")
        ids = list(ids)
        rows = self._prepare(embeddings)
        if rows.shape[0] != len(ids):
            raise ValueError(f"{rows.shape[0]} embeddings for {len(ids)} ids")
        tags = None if item_categories is None else self._item_tags(item_categories, len(ids))
        known: Dict[str, int] = {}     # id -> its last row in the call (positions stay unique)
        unknown: Dict[str, int] = {}   # in order of first appearance, the last row wins too
        for i, item_id in enumerate(ids):
            (known if item_id in self.reverse_id_map else unknown)[item_id] = i
        if known:
            take = torch.tensor(list(known.values()), dtype=torch.int64, device=rows.device)
            pos = torch.tensor([self.reverse_id_map[i] for i in known], dtype=torch.int64, device=rows.device)
            new_rows = self._to_storage(rows[take])
            with self._searcher_lock():   # row and tags under one acquisition: a search sees both or neither
                kernels.scatter_rows(new_rows, pos, self.index)
                if tags is not None:
                    self._tags_write([self.reverse_id_map[i] for i in known], tags[list(known.values())])
        if unknown:
            take = torch.tensor(list(unknown.values()), dtype=torch.int64, device=rows.device)
            self._append(rows[take], list(unknown), None if tags is None else tags[list(unknown.values())])
        logger.info("Updated %d items in place, appended %d. Total size: %d", len(known), len(unknown),
                    self.current_size)

    def remove(self, ids: List[str]) -> Optional[int]:
        """retrieval.py:239-246: a no-op with a warning, like the reference, unless
        the index is ``mutable``. Then every row stored under one of ``ids`` leaves
        and later rows shift down in order (``faiss.IndexFlat.remove_ids``);
        unknown ids are ignored. Returns the number of rows removed."""
        if not self.mutable:
            logger.warning("Flat index doesn't support removal. Consider periodic rebuilds.")
            return None
        if self.index is None:
            raise ValueError("Index not built yet")
        hit = {i for i in ids if i in self.reverse_id_map}
        if not hit:
            return 0
        n = self.current_size
        keep = np.ones(n, dtype=bool)
        keep[[self.reverse_id_map[i] for i in hit]] = False
        unnamed = self._ids.count(None)
        if n - unnamed != len(self.reverse_id_map):
            # an id stored more than once through add: every one of its rows goes
            keep[[p for p, i in enumerate(self._ids) if i in hit]] = False
        # bit j of word w = row 32w + j (little-endian bytes of little-endian words)
        bits = np.packbits(keep, bitorder="little")
        words = np.zeros(-(-n // 32), dtype="<u4")
        words.view(np.uint8)[: bits.size] = bits
        d_bits = torch.from_numpy(words.view(np.int32)).to(self._dev())
        buf = torch.empty_like(self.index)  # the old capacity
        # the O(N) host side: the surviving ids as the runs between removed rows (list
        # slices, not a per-row loop), then both maps in ascending position — the last
        # row of an id names it, as add leaves it
        old_ids, new_ids, a = self._ids, [], 0
        for r in np.flatnonzero(~keep).tolist():
            new_ids.extend(old_ids[a:r])
            a = r + 1
        new_ids.extend(old_ids[a:])
        if unnamed:
            id_map = {p: i for p, i in enumerate(new_ids) if i is not None}
            reverse_id_map = {i: p for p, i in id_map.items()}
        else:
            id_map = dict(enumerate(new_ids))
            reverse_id_map = dict(zip(new_ids, range(len(new_ids))))
        with self._searcher_lock():
            kernels.rows_compact(self.index[:n], d_bits, buf)
            if self._tags is not None:   # the tags shift down with the rows
                kept = self._tags[:n][torch.from_numpy(keep).to(self._dev())]
                self._tags = torch.zeros_like(self._tags)
                self._tags[: kept.numel()] = kept
            self.index = buf
            self.current_size = len(new_ids)    # the host's own count: no device read
            self._ids, self.id_map, self.reverse_id_map = new_ids, id_map, reverse_id_map
            self._generation += 1               # the rows moved: resident searchers drop their graphs
        logger.info("Removed %d items from index. Total size: %d", n - self.current_size, self.current_size)
        return n - self.current_size

    def vectors(self) -> np.ndarray:
        if self.index is None:
            return np.zeros((0, self.dimension), np.float32)
        return self.index[: self.current_size, : self.dimension].float().cpu().numpy()

    def save(self, path: str):
        """retrieval.py:248-273: ``<path>.faiss`` (IndexFlatIP/IndexFlatL2 binary
        layout: fourcc, header, code vector) + ``<path>.pkl`` id maps."""
        if self.index is None:
            raise ValueError("No index to save")
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        write_flat_index(path.with_suffix(".faiss"), self.vectors(), not self._l2)
        self._save_ids(path)
        self._save_tags(path)
        logger.info("Saved index to %s", path)

    def load(self, path: str):
        """retrieval.py:275-299."""
        path = Path(path)
        vecs, _ip = read_flat_index(path.with_suffix(".faiss"))
        data = self._read_pkl(path)
        self.config = data.get("config", self.config)
        self.metric = self.config.get("metric", self.metric)
        self._l2 = self.metric not in ("cosine", "inner_product")
        self.mutable = bool(self.config.get("mutable", False))
        self.dimension = vecs.shape[1]
        self.index = None
        self.current_size = 0
        self._store(torch.from_numpy(vecs).to(self._dev()))
        self.current_size = int(data["current_size"])
        self._load_ids(data, self.current_size)
        self._load_tags(path)
        self._generation += 1
        self._online = None  # load may change the dimension and the metric
        logger.info("Loaded index from %s with %d items", path, self.current_size)


# Faiss 1.7.x binary layout of IndexFlat (restated from the published format:
# fourcc, d:int32, ntotal:int64, 2 x dummy int64, is_trained:bool, metric:int32,
# then the code vector as a size_t count of floats followed by the floats).
_FOURCC_IP = b"IxFI"
_FOURCC_L2 = b"IxF2"


def write_flat_index(path: Path, vecs: np.ndarray, inner_product: bool = True):
    vecs = np.ascontiguousarray(vecs, dtype=np.float32)
    n, d = vecs.shape
    with open(path, "wb") as f:
        f.write(_FOURCC_IP if inner_product else _FOURCC_L2)
        f.write(struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 0 if inner_product else 1))
        f.write(struct.pack("<Q", n * d))
        f.write(vecs.tobytes())


def read_flat_index(path: Path) -> Tuple[np.ndarray, bool]:
    with open(path, "rb") as f:
        four = f.read(4)
        if four not in (_FOURCC_IP, _FOURCC_L2):
            raise ValueError(f"{path}: not a flat index (fourcc {four!r})")
        d, n, _, _, _, _metric = struct.unpack("<iqqq?i", f.read(struct.calcsize("<iqqq?i")))
        (cnt,) = struct.unpack("<Q", f.read(8))
        if cnt != n * d:
            raise ValueError(f"{path}: corrupt code vector ({cnt} != {n}*{d})")
        vecs = np.frombuffer(f.read(cnt * 4), dtype=np.float32).reshape(n, d).copy()
    return vecs, four == _FOURCC_IP


@contextlib.contextmanager
def _capture(graph: "torch.cuda.CUDAGraph"):
    """``torch.cuda.graph(graph, capture_error_mode="thread_local")`` with the
    cyclic garbage collector paused. A collection that starts inside the
    capture may finalise a dead cycle that holds device objects — a dropped
    index and its resident searcher refer to each other, with pinned buffers
    and captured graphs — and freeing those is not a capturable call: the
    process aborts. torch does not collect before a capture
    (``torch.compiler.config.force_cudagraph_gc`` is off by default), so such a
    cycle simply waits for the first collection after the capture."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            yield
    finally:
        if was_enabled:
            gc.enable()


class OnlineSearcher:
    """Resident small-batch searcher over one :class:`HipFlatIPIndex`
    (``index.online_searcher(max_batch)``): the per-request shape of the
    reference's serving path (src/serving/service.py:268-302 →
    retrieval.py:141-197, one user embedding per call).

    It owns, allocated once: pinned host buffers for the queries
    ``[max_batch, d]`` fp32 and for scores / positions ``[max_batch, 128]``,
    the matching device buffers, and the top-K workspace. A call is a host
    copy into the pinned query buffer, ONE replay of a captured graph (H2D
    copy → ``l2_renorm`` for the cosine metric → storage-dtype cast →
    ``rt_flatip_topk_online`` → D2H copies: a straight chain, the same
    arithmetic in the same order as ``HipFlatIPIndex.search_tensors``) and one
    stream synchronise. Graphs are captured lazily per (nq, k), the first call
    at a shape running the sequence eagerly; at most 32 are kept, the oldest
    dropped. ``RTREC_ONLINE_GRAPH=0`` (read at every call) runs the sequence
    eagerly instead. After the first call at a given (nq, k) a call makes no
    torch allocation.

    Exclusion lists (``search(q, k, exclude=...)``, ``max_exclude`` entries per
    call, default 8,192): pinned CSR buffers (``offsets [max_batch + 1]``,
    ``items [max_exclude]``) and their device twins are allocated here too; a
    call with lists replays a graph keyed (nq, k, True) whose chain carries two
    fixed-size H2D copies of them in front of ``rt_flatip_topk_online_lists``
    — the lists are data, so one graph serves every list length.

    MMR re-rank (``search(q, k, mmr=(k_out, lam))``): a second device pair for the
    re-ranked scores / positions and a pinned ``[max_batch]`` lambda buffer with
    its device twin are allocated here too; such a call replays a graph whose key
    ends in ``("mmr", k_out)`` and whose chain carries one fixed-size H2D copy of
    lambda and, after the scan, ``rt_mmr_rerank`` — lambda is data, so one graph
    serves every value; the keys of calls without ``mmr`` are unchanged.

    The searcher holds the index's row pointer and size: ``build`` / ``add`` /
    ``load`` / ``remove`` bump the index's generation, and a searcher that finds
    its generation stale drops its graphs and captures again. An in-place
    ``update`` of a ``mutable`` index moves nothing and bumps nothing: the
    graphs stay and read the new row at their next replay.

    Thread safety: calls are serialised by ``lock`` (re-entrant). ``search``
    returns views of the searcher's own host buffers, valid until the next
    call — a caller sharing the searcher between threads reads them while
    holding ``lock``. The first call at a new (nq, k) captures its graph in
    ``thread_local`` capture mode, so other threads may do CUDA work meanwhile.
    """

    MAX_BATCH = kernels.ONLINE_MAX_NQ
    MAX_K = kernels.ONLINE_MAX_K
    MAX_GRAPHS = 32

    def __init__(self, index: "HipFlatIPIndex", max_batch: int = 8, max_exclude: int = 8192):
        if not 1 <= int(max_batch) <= self.MAX_BATCH:
            raise ValueError(f"max_batch={max_batch}: 1..{self.MAX_BATCH}")
        if int(max_exclude) < 0:
            raise ValueError(f"max_exclude={max_exclude}: 0 or more entries per call")
        if index._l2:
            raise ValueError("OnlineSearcher serves the inner-product metrics ('cosine', 'inner_product')")
        self.index = index
        self.max_batch = int(max_batch)
        self.max_exclude = int(max_exclude)
        self.lock = threading.RLock()
        dev, d, mb = index._dev(), index.dimension, self.max_batch
        self._h_q = torch.empty((mb, d), dtype=torch.float32).pin_memory()
        self._h_s = torch.empty(mb * self.MAX_K, dtype=torch.float32).pin_memory()
        self._h_p = torch.empty(mb * self.MAX_K, dtype=torch.int64).pin_memory()
        self._h_s_np, self._h_p_np = self._h_s.numpy(), self._h_p.numpy()
        self._d_q32 = torch.empty((mb, d), dtype=torch.float32, device=dev)
        self._d_q = self._d_q32 if index.storage_dtype == torch.float32 else \
            torch.empty((mb, d), dtype=index.storage_dtype, device=dev)
        self._d_s = torch.empty(mb * self.MAX_K, dtype=torch.float32, device=dev)
        self._d_p = torch.empty(mb * self.MAX_K, dtype=torch.int64, device=dev)
        # the largest workspace any corpus size asks for: [mb][128][512 blocks] keys
        self._ws = torch.empty(mb * self.MAX_K * 512 * 8, dtype=torch.uint8, device=dev)
        # the per-call exclusion lists, a CSR over the call's queries: row q = query q
        self._h_xo = torch.zeros(mb + 1, dtype=torch.int64).pin_memory()
        self._h_xi = torch.zeros(max(self.max_exclude, 1), dtype=torch.int32).pin_memory()
        self._h_xo_np, self._h_xi_np = self._h_xo.numpy(), self._h_xi.numpy()
        self._d_xo = torch.zeros(mb + 1, dtype=torch.int64, device=dev)
        self._d_xi = torch.zeros(max(self.max_exclude, 1), dtype=torch.int32, device=dev)
        # the per-call category masks: any_of [mb] then none_of [mb], one fixed-size H2D copy
        self._h_tm = torch.zeros(2 * mb, dtype=torch.int64).pin_memory()
        self._h_tm_np = self._h_tm.numpy()
        self._d_tm = torch.zeros(2 * mb, dtype=torch.int64, device=dev)
        self._item_tags: Optional[torch.Tensor] = None   # the index's resident tags (per generation)
        # the MMR re-rank: its output pair (the scan's stays its input), and lambda [mb] — data,
        # one fixed-size H2D copy, so one graph serves every value
        self._d_s2 = torch.empty(mb * self.MAX_K, dtype=torch.float32, device=dev)
        self._d_p2 = torch.empty(mb * self.MAX_K, dtype=torch.int64, device=dev)
        self._h_lam = torch.zeros(mb, dtype=torch.float32).pin_memory()
        self._h_lam_np = self._h_lam.numpy()
        self._d_lam = torch.zeros(mb, dtype=torch.float32, device=dev)
        self._mmr_ops = None   # (rows, pos_slot, n_pos) of the index, per generation, made at the first re-ranked call
        # keys (nq, k) without lists — as before lists existed — and (nq, k, True) with
        self._graphs: "OrderedDict[tuple, torch.cuda.CUDAGraph]" = OrderedDict()
        self._generation = -1
        self._rows: Optional[torch.Tensor] = None

    def _upload(self, nq: int):
        """H2D copy of the pinned queries into the fp32 device query rows."""
        self._d_q32[:nq].copy_(self._h_q[:nq], non_blocking=True)

    def _stage_lists(self, nq: int, exclude) -> bool:
        """Write ``exclude`` (per query: ascending unique positions, int arrays) into
        the pinned CSR. False when the call holds more than ``max_exclude`` entries."""
        total = sum(len(e) for e in exclude)
        if total > self.max_exclude:
            return False
        o = 0
        self._h_xo_np[0] = 0
        for q in range(nq):
            n = len(exclude[q])
            self._h_xi_np[o:o + n] = exclude[q]
            o += n
            self._h_xo_np[q + 1] = o
        self._h_xo_np[nq + 1:] = o
        return True

    def _upload_lists(self):
        """The two fixed-size H2D copies of the per-call lists: whole buffers, so that
        one captured graph serves every list length."""
        self._d_xo.copy_(self._h_xo, non_blocking=True)
        self._d_xi.copy_(self._h_xi, non_blocking=True)

    def _list_source(self):
        """The per-call lists as a source of ``kernels.flatip_topk_online(exclude_lists=...)``."""
        return (self._d_xo, self._d_xi)

    def _tag_filter(self, nq: int):
        """The per-call masks over the index's resident tags, as ``tag_filter`` of the kernels."""
        mb = self.max_batch
        return (self._item_tags, self._d_tm[:nq], self._d_tm[mb:mb + nq])

    def _stage_tags(self, nq: int, tags):
        """Write ``tags = (any_of, none_of)`` into the pinned mask buffer."""
        if self.index.categories is None or self._item_tags is None:
            self.index._need_categories("tags")
            raise ValueError("the index holds no tags yet")
        if len(tags) != 2:
            raise ValueError("tags is (any_of, none_of)")
        mb = self.max_batch
        for at, m in zip((0, mb), tags):
            w = _mask_words(m, nq)
            self._h_tm_np[at:at + nq] = 0 if w is None else w

    def _device_chain(self, nq: int, k: int, sources=None, tags: bool = False):
        """``_d_q32[:nq]`` (fp32 device rows, however they got there: ``_upload``,
        or a kernel that wrote them — :class:`rtrec_amd.serving.online.OnlineRecommender`)
        -> ``l2_renorm`` for the cosine metric (in place) -> storage-dtype cast ->
        ``rt_flatip_topk_online`` (``sources``: ``rt_flatip_topk_online_lists`` with
        these exclusion sources; ``tags``: ``rt_flatip_topk_online_tags`` with the
        uploaded masks too) into the device scores / positions."""
        n = nq * k
        q32 = self._d_q32[:nq]
        if self.index.metric == "cosine":
            kernels.l2_renorm_(q32)
        q = self._d_q[:nq]
        if q.data_ptr() != q32.data_ptr():
            q.copy_(q32)
        kernels.flatip_topk_online(q, self._rows, k, out=(self._d_s[:n].view(nq, k), self._d_p[:n].view(nq, k)),
                                   workspace_buf=self._ws, exclude_lists=sources or None,
                                   tag_filter=self._tag_filter(nq) if tags else None)

    def _stage_mmr(self, nq: int, lam):
        """Write lambda (one float, or one per query) into the pinned buffer, and make
        the index's re-rank operands when this generation has none yet. Under ``lock``,
        after ``_revalidate``."""
        lam = np.asarray(lam, dtype=np.float32).reshape(-1)
        if lam.size not in (1, nq):
            raise ValueError(f"{lam.size} mmr lambdas for {nq} queries")
        if not bool(np.all((lam >= 0) & (lam <= 1))):
            raise ValueError(f"mmr lambda {lam.tolist()}: 0 <= lambda <= 1")
        self._h_lam_np[:nq] = lam
        if self._mmr_ops is None:
            self._mmr_ops = self.index._mmr_operands()

    def _device_mmr(self, nq: int, k: int, k_out: int):
        """``rt_mmr_rerank`` of the device scores / positions ``[nq, k]`` the chain wrote
        into the second device pair ``[nq, k_out]``, lambda from ``_d_lam``."""
        n, m = nq * k, nq * k_out
        rows, pos_slot, n_pos = self._mmr_ops
        kernels.mmr_rerank(self._d_s[:n].view(nq, k), self._d_p[:n].view(nq, k), rows, k_out, self._d_lam,
                           pos_slot=pos_slot, n_pos=n_pos, normalize=self.index.metric != "cosine",
                           out=(self._d_s2[:m].view(nq, k_out), self._d_p2[:m].view(nq, k_out)))

    def _download(self, nq: int, k: int, mmr: bool = False):
        """D2H copies of scores and positions into the pinned result buffers (``mmr``:
        of the re-ranked pair)."""
        n = nq * k
        self._h_s[:n].copy_((self._d_s2 if mmr else self._d_s)[:n], non_blocking=True)
        self._h_p[:n].copy_((self._d_p2 if mmr else self._d_p)[:n], non_blocking=True)

    def _sequence(self, nq: int, k: int, lists: bool = False, tags: bool = False, mmr_k: int = 0):
        """The stream-ordered chain of one call, on torch's current stream (``mmr_k``:
        then ``rt_mmr_rerank`` of the k candidates into ``mmr_k`` results)."""
        self._upload(nq)
        if lists:
            self._upload_lists()
        if tags:
            self._d_tm.copy_(self._h_tm, non_blocking=True)   # whole buffer: the masks are data
        if mmr_k:
            self._d_lam.copy_(self._h_lam, non_blocking=True)   # whole buffer: lambda is data
        self._device_chain(nq, k, [self._list_source()] if lists else None, tags=tags)
        if mmr_k:
            self._device_mmr(nq, k, mmr_k)
            self._download(nq, mmr_k, True)
        else:
            self._download(nq, k)

    def _graph_key(self, nq: int, k: int, lists: bool) -> tuple:
        """What one captured graph serves (a call with category masks: this key + ("tags",))."""
        return (nq, k, True) if lists else (nq, k)

    def _revalidate(self) -> bool:
        """Under ``lock``: pick up the index's rows again when ``build`` / ``add`` /
        ``load`` moved or grew them (the graphs hold stale pointers: dropped).
        True when they were stale."""
        idx = self.index
        if self._generation == idx._generation:
            return False
        self._graphs.clear()
        if idx._l2 or idx.dimension != self._h_q.shape[1] or idx.storage_dtype != self._d_q.dtype:
            # a load changed what the buffers were sized and checked for
            raise ValueError("the index changed its dimension, metric or storage dtype since this "
                             "searcher was made: obtain a new one (index.online_searcher)")
        self._rows = idx.index[: idx.current_size]
        self._item_tags = idx._tags
        self._mmr_ops = None
        self._generation = idx._generation
        return True

    def search(self, query_embeddings: Array, k: int, exclude=None, tags=None, mmr=None
               ) -> Tuple[np.ndarray, np.ndarray]:
        """(scores [nq, k] f32, positions [nq, k] int64, (-FLT_MAX, -1) padded) as
        numpy views of the searcher's pinned buffers: valid until the next call.

        ``exclude``: ``nq`` sequences of corpus positions that query q must not
        return (sorted and de-duplicated here; positions outside the corpus are
        ignored). They travel as data through two fixed-size H2D copies in front of
        the scan, which reads them itself (``rt_flatip_topk_online_lists``): one
        graph per (nq, k) serves every list length up to ``max_exclude`` entries
        per call. A call with more takes the non-resident path — a dense bitmap
        and ``search_tensors(..., exclude_bits=...)`` — and returns the same result
        in fresh arrays. ``exclude=None`` replays the graphs of a searcher without
        lists.

        ``tags=(any_of, none_of)``: per-query 64-bit category masks (uint64 / int64
        ``[nq]``; either may be None) over the index's resident tags; the scan
        tests eligibility itself. The masks travel through one more fixed-size
        H2D copy, and one graph per (nq, k, lists, tags) serves every mask value
        and, the tags being read at replay, every in-place tag change.

        ``mmr=(k_out, lam)``: the k results of the scan are candidates, and
        ``rt_mmr_rerank`` — one more launch at the end of the chain, over the index's
        stored rows — chooses ``k_out <= k`` of them into a second pre-allocated
        device pair, which is what is downloaded: the returned views are
        ``[nq, k_out]``, in selection order, with the original scores. ``lam`` (one
        float or one per query, in [0, 1]) travels through a pinned ``[max_batch]``
        buffer and one fixed-size H2D copy; the graph key gains ``("mmr", k_out)`` at
        its end, so one graph serves every lambda. The position-to-row map: none for
        a Flat index, the resident ``pos_slot`` of a :class:`HipMutableIVFFlatIndex`
        (an in-place ``update`` keeps the graph; the replay reads the new row and the
        new slot), and for a :class:`HipIVFFlatIndex` the inverse of ``row_pos``,
        made once per generation at the first re-ranked call."""
        idx = self.index
        if idx.index is None:
            raise ValueError("Index not built yet")
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"k={k}: the online searcher returns 1..{self.MAX_K} results per query")
        t = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.as_tensor(query_embeddings)
        if t.dim() == 1:
            t = t.reshape(1, -1)
        nq = t.shape[0]
        if t.dim() != 2 or not 1 <= nq <= self.max_batch:
            raise ValueError(f"{nq} queries: the online searcher takes 1..{self.max_batch}")
        if t.shape[1] != idx.dimension:
            raise ValueError(f"expected dimension {idx.dimension}, got {t.shape[1]}")
        lists = exclude is not None
        if lists:
            if len(exclude) != nq:
                raise ValueError(f"exclude holds {len(exclude)} lists for {nq} queries")
            exclude = [_sorted_positions(e, idx.current_size) for e in exclude]
        tagged = tags is not None
        mmr_k = 0
        if mmr is not None:
            mmr_k, lam = int(mmr[0]), mmr[1]
            if not 1 <= mmr_k <= k:
                raise ValueError(f"mmr: {mmr_k} results of {k} candidates: 1 <= k_out <= k")
        with self.lock:
            self._revalidate()
            if tagged:
                self._stage_tags(nq, tags)
            if mmr_k:
                self._stage_mmr(nq, lam)
            if lists and not self._stage_lists(nq, exclude):
                # more entries than the resident buffers hold: the dense bitmap of the default path
                bits = kernels.exclusion_bitmap(nq, idx.current_size, exclude, self._d_s.device)
                s, p = idx.search_tensors(t, k, exclude_bits=bits, tag_filter=tags)
                if mmr_k:
                    s, p = idx.mmr_rerank_tensors(s, p, mmr_k, self._d_lam.copy_(self._h_lam))
                return s.cpu().numpy(), p.cpu().numpy()
            self._h_q[:nq].copy_(t)
            key = self._graph_key(nq, k, lists) + (("tags",) if tagged else ()) + (("mmr", mmr_k) if mmr_k else ())
            stream = torch.cuda.current_stream(self._d_s.device)
            if os.environ.get("RTREC_ONLINE_GRAPH", "1") == "0":
                self._sequence(nq, k, lists, tagged, mmr_k)
            else:
                g = self._graphs.get(key)
                if g is not None:
                    g.replay()
                else:
                    # the first call at this shape: its answer comes from an eager run
                    # (which also loads every kernel), then the chain is captured —
                    # a capture executes nothing, the host buffers keep the answer
                    self._sequence(nq, k, lists, tagged, mmr_k)
                    stream.synchronize()
                    g = torch.cuda.CUDAGraph()
                    # thread_local: CUDA work of other threads (an allocation, a default-path
                    # search) during the capture neither enters it nor invalidates it
                    with _capture(g):
                        self._sequence(nq, k, lists, tagged, mmr_k)
                    while len(self._graphs) >= self.MAX_GRAPHS:
                        self._graphs.popitem(last=False)
                    self._graphs[key] = g
            stream.synchronize()
            k = mmr_k or k
            return self._h_s_np[:nq * k].reshape(nq, k), self._h_p_np[:nq * k].reshape(nq, k)


class HipShardedFlatIPIndex(_HbmIndex):
    """The same ``IndexBase`` contract as :class:`HipFlatIPIndex` (FaissIndex
    ``Flat``, retrieval.py:49-329) over a corpus ROW-SHARDED across the ranks
    of a process group, one shard in each GPU's HBM.

    It is an SPMD object: every rank constructs it and makes the same calls
    with the same arguments (``build``/``add`` with the whole batch of rows,
    ``search`` with the same queries), like every collective API, and every
    rank gets the full result.

    * **Layout.** Global positions follow build order, then add order, exactly
      as in one :class:`HipFlatIPIndex` (so results are equal id for id).
      ``build`` keeps rank r's contiguous slice ``shard_range(N, world, r)``;
      each ``add`` of m rows appends to every rank the slice
      ``shard_range(m, world, r)`` of the new global rows, so shards stay
      balanced. A rank's rows stay in increasing global order (an ``int64``
      position map on the device once an add made them non-contiguous), so the
      kernels' lower-id-wins tie rule holds globally.
    * **Search** (:func:`rtrec_amd.dist.sharded.sharded_topk_global`): one
      corpus-wide threshold per query from the ranks' shard samples, each
      rank's rows at or above it, all-to-all + owner merge
      (``rt_topk_merge``), one all-gather of the merged slices (``layout="all"``,
      the IndexBase ``search``) — or each rank only its slice of the queries
      (``layout="owner"``, :meth:`search_tensors`, what ``bench.py`` times).
      Shapes without the 16-bit v4 plan (float32 storage, k > 128) take the
      plain form of the same exchange. Queries run in tiles of
      ``query_tile`` (65,536) rows.
    * **string ids**: the id map is replicated on every rank (host data).
      ``filter_ids`` over-fetches ``k_search = min(2k, N)`` like FaissIndex
      (retrieval.py:170-195); -1 padding is dropped; k <= 512.
    * **save/load**: each rank writes its own ``<path>.shard{r}of{W}.faiss``
      (IndexFlat layout) and ``.pos.npy`` (its global positions); rank 0 writes
      the ``<path>.pkl`` id maps. ``load`` on the same world size reads only
      this rank's files; on another world size (or from a single-GPU
      :class:`HipFlatIPIndex` save, ``<path>.faiss``) it re-shards.

    Config keys: those of :class:`HipFlatIPIndex` for the inner-product
    metrics ("cosine", "inner_product"), plus ``process_group`` (default: the
    default group; world 1 without one) and ``query_tile``. The ``mutable``
    option of :class:`HipFlatIPIndex` is not served here yet: ``update`` and
    ``remove`` keep the reference's warning stubs (a cross-rank compaction has
    to re-balance the shards). Nor is ``exclude_ids``: ``search`` here takes the
    allow-list ``filter_ids`` only.
    """

    MAX_K = 512  # rt_topk_merge: k_out <= 512

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(dict(config or {}))
        self.index_factory = self.config.get("index_factory", "Flat")
        self.nprobe = self.config.get("nprobe", 20)
        self.group = self.config.pop("process_group", None)
        self.query_tile = int(self.config.get("query_tile", 65536))
        from ..dist import sharded as _sh
        self._sh = _sh
        self.world, self.rank = _sh._world(self.group)
        self._reset()

    def _check_metric(self):
        if self._l2:
            raise ValueError("the sharded index serves the inner-product metrics ('cosine', 'inner_product'); "
                             "IndexFlatL2 is the single-GPU HipFlatIPIndex")

    _NO_CATEGORIES = ("the sharded index does not serve category filters: use a single-GPU index "
                      "(HipFlatIPIndex, HipIVFFlatIndex, HipMutableIVFFlatIndex)")

    def _check_categories(self):
        raise ValueError("categories: " + self._NO_CATEGORIES)

    def set_item_categories(self, ids, item_categories):
        raise ValueError(self._NO_CATEGORIES)

    # -- hooks (the CPU orchestration tests substitute these, and the base's _dev
    # and _renorm_) -----------------------------------------------------------
    def _ops(self, rows: torch.Tensor):
        return self._sh.ShardOps(rows, self.begin, self.gpos)

    def _merge(self, s, i, k):
        return kernels.topk_merge(s, i, k)

    # -- layout --------------------------------------------------------------
    def _reset(self):
        self.shard: Optional[torch.Tensor] = None  # [capacity, d] storage rows; first n_local valid
        self.n_local = 0
        self.begin = 0                             # global position of local row 0 (contiguous shard)
        self.gpos: Optional[torch.Tensor] = None   # int64 [n_local] global positions once non-contiguous
        self.shard_sizes: List[int] = [0] * self.world
        self._reset_ids()
        self._implicit_ids = False                 # build_shard without ids: id = str(position)
        self.current_size = 0

    def _append_local(self, rows: torch.Tensor, positions: Optional[torch.Tensor]):
        """Append prepared rows (their global positions: ``positions``, or the
        contiguous run after the current ones when None)."""
        rows = rows.to(self.storage_dtype)
        n_new = self.n_local + rows.shape[0]
        if self.shard is None or self.shard.shape[0] < n_new:
            cap = max(n_new, 2 * (self.shard.shape[0] if self.shard is not None else 0), 1024)
            buf = torch.empty((cap, self.dimension), dtype=self.storage_dtype, device=self._dev())
            if self.shard is not None and self.n_local:
                buf[: self.n_local].copy_(self.shard[: self.n_local])
            self.shard = buf
        self.shard[self.n_local:n_new].copy_(rows)
        if positions is not None:
            if self.gpos is None:
                self.gpos = torch.arange(self.begin, self.begin + self.n_local, dtype=torch.int64,
                                         device=self._dev())
            self.gpos = torch.cat([self.gpos, positions.to(device=self._dev(), dtype=torch.int64)])
        self.n_local = n_new

    # -- IndexBase -------------------------------------------------------------
    def build(self, embeddings: Array, ids: List[str]):
        """retrieval.py:70-139 (Flat): every rank passes the whole corpus and
        keeps its slice."""
        start = time.time()
        n = len(embeddings)
        self._reset()
        b, c = self._sh.shard_range(n, self.world, self.rank)
        self.begin = b
        self._append_local(self._prepare(embeddings[b:b + c]), None)
        self.shard_sizes = [self._sh.shard_range(n, self.world, r)[1] for r in range(self.world)]
        self._record_ids(0, ids, n)
        self.current_size = n
        logger.info("Sharded index built in %.2f seconds (%d of %d rows on rank %d)", time.time() - start, c, n,
                    self.rank)

    def build_shard(self, rows: Array, n_total: int, ids: Optional[List[str]] = None, prepared: bool = False):
        """Rank-local build: this rank passes only ITS slice
        ``shard_range(n_total, world, rank)`` of the corpus (e.g. rows that
        already live on its GPU). ``prepared``: the rows are already
        normalised (no renorm)."""
        self._reset()
        b, c = self._sh.shard_range(n_total, self.world, self.rank)
        if len(rows) != c:
            raise ValueError(f"rank {self.rank} holds {len(rows)} rows, shard_range says {c}")
        self.begin = b
        if prepared:
            t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows)
            self._append_local(t.to(self._dev()), None)
        else:
            self._append_local(self._prepare(rows), None)
        self.shard_sizes = [self._sh.shard_range(n_total, self.world, r)[1] for r in range(self.world)]
        if ids is None:  # string ids = positions, materialised only when needed (add / save / load)
            self._implicit_ids = True
        else:
            self._record_ids(0, ids, n_total)
        self.current_size = int(n_total)
        return self

    def _materialize_ids(self):
        if self._implicit_ids:
            self._implicit_ids = False
            self._record_ids(0, [str(i) for i in range(self.current_size)], self.current_size)

    def add(self, embeddings: Array, ids: List[str]):
        """retrieval.py:199-226: every rank passes the whole batch; the new
        global rows current_size.. are spread over the ranks (shard_range of
        the batch), each rank appending its slice."""
        if self.shard is None:
            raise ValueError("Index not built yet")
        self._materialize_ids()
        m = len(embeddings)
        b, c = self._sh.shard_range(m, self.world, self.rank)
        pos = torch.arange(self.current_size + b, self.current_size + b + c, dtype=torch.int64)
        self._append_local(self._prepare(embeddings[b:b + c]), pos)
        self.shard_sizes = [s + self._sh.shard_range(m, self.world, r)[1] for r, s in enumerate(self.shard_sizes)]
        self._record_ids(self.current_size, ids, m)
        self.current_size += m
        logger.info("Added %d items to index. Total size: %d", m, self.current_size)

    def update(self, embeddings: Array, ids: List[str]):
        logger.warning("Flat index doesn't support direct updates. Consider periodic rebuilds.")

    def remove(self, ids: List[str]):
        logger.warning("Flat index doesn't support removal. Consider periodic rebuilds.")

    def search_tensors(self, query_embeddings: Array, k: int, layout: str = "all", prepared: bool = False
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores [nq, k], global positions [nq, k]) with (-FLT_MAX, -1)
        padding. ``layout="all"``: every rank gets every query's result;
        ``"owner"``: each rank gets its slice ``shard_range(tile, world, rank)``
        of every query tile (nq % world == 0). ``prepared``: the queries are a
        device tensor already normalised and in the storage dtype (no copy)."""
        if self.shard is None:
            raise ValueError("Index not built yet")
        if not 0 < k <= self.MAX_K:
            raise ValueError(f"k={k}: the sharded index returns 1..{self.MAX_K} results per query")
        if layout not in ("all", "owner"):
            raise ValueError(f"layout {layout!r}")
        if prepared:
            q = query_embeddings
            if q.dtype != self.storage_dtype or q.dim() != 2 or q.shape[1] != self.dimension:
                raise ValueError("prepared queries must be [nq, dimension] in the storage dtype")
        else:
            q = self._prepare(query_embeddings).to(self.storage_dtype)
        owner = layout == "owner"
        if owner and q.shape[0] % self.world:
            raise ValueError(f"{q.shape[0]} queries do not split over {self.world} ranks")
        tile = max(self.query_tile - self.query_tile % self.world, self.world)
        ops = self._ops(self.shard[: self.n_local])
        parts_s, parts_i = [], []
        for t0 in range(0, max(q.shape[0], 1), tile):
            qt = q[t0:t0 + tile]
            if qt.shape[0] == 0:
                break
            s, i = self._sh.sharded_topk_global(qt, k, self.current_size, ops, self._merge, self.group,
                                                owner=owner, shard_rows=self.shard_sizes)
            parts_s.append(s)
            parts_i.append(i)
        if not parts_s:
            return (torch.empty((0, k), dtype=torch.float32, device=q.device),
                    torch.empty((0, k), dtype=torch.int64, device=q.device))
        if len(parts_s) == 1:
            return parts_s[0], parts_i[0]
        return torch.cat(parts_s), torch.cat(parts_i)

    _NO_MMR = ("the sharded index does not serve the MMR re-rank (a candidate's row may live on another rank): "
               "use a single-GPU index (HipFlatIPIndex, HipIVFFlatIndex, HipMutableIVFFlatIndex)")

    def _check_mmr(self):
        raise ValueError("mmr_lambda: " + self._NO_MMR)

    def search(self, query_embeddings: Array, k: int = 10,
               filter_ids: Optional[List[str]] = None, filter_categories=None, exclude_categories=None,
               mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None
               ) -> Tuple[List[List[str]], List[List[float]]]:
        """retrieval.py:141-197 on every rank (collective). Category filters are not
        served here: ``filter_categories`` / ``exclude_categories`` raise, and so do
        ``mmr_lambda`` / ``mmr_candidates``."""
        if filter_categories is not None or exclude_categories is not None:
            raise ValueError(self._NO_CATEGORIES)
        if mmr_lambda is not None or mmr_candidates is not None:
            raise ValueError(self._NO_MMR)
        if self.shard is None:
            raise ValueError("Index not built yet")
        k_search = min(k * 2, self.current_size) if filter_ids else k
        if k_search <= 0:
            n = 1 if np.ndim(query_embeddings) == 1 else len(query_embeddings)
            return [[] for _ in range(n)], [[] for _ in range(n)]
        scores, pos = self.search_tensors(query_embeddings, k_search)
        id_map = _PositionIds(self.current_size) if self._implicit_ids else self.id_map
        return _lists_from_positions(scores.cpu().numpy(), pos.cpu().numpy(), id_map, k, filter_ids)

    def vectors(self) -> np.ndarray:
        """This rank's rows (fp32, global order)."""
        if self.shard is None:
            return np.zeros((0, self.dimension), np.float32)
        return self.shard[: self.n_local].float().cpu().numpy()

    def positions(self) -> np.ndarray:
        """Global positions of this rank's rows."""
        if self.gpos is not None:
            return self.gpos.cpu().numpy()
        return np.arange(self.begin, self.begin + self.n_local, dtype=np.int64)

    def _shard_files(self, path: Path, r: int, w: int) -> Tuple[Path, Path]:
        """(rows .faiss, positions .npy) of shard r of w, next to ``path``."""
        stem = path.with_suffix("").name
        return (path.with_name(f"{stem}.shard{r}of{w}.faiss"), path.with_name(f"{stem}.shard{r}of{w}.pos.npy"))

    def _barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier(group=self.group)

    def save(self, path: str):
        """Per-shard save: ``<path>.shard{r}of{W}.faiss`` + ``.pos.npy`` on every
        rank, ``<path>.pkl`` (id maps, layout) from rank 0 (retrieval.py:248-273)."""
        if self.shard is None:
            raise ValueError("No index to save")
        self._materialize_ids()
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        fx, fp = self._shard_files(path, self.rank, self.world)
        write_flat_index(fx, self.vectors(), True)
        with open(fp, "wb") as f:
            np.save(f, self.positions(), allow_pickle=False)
        if self.rank == 0:
            self._save_ids(path, world=self.world, shard_sizes=self.shard_sizes)
        self._barrier()
        logger.info("Saved shard %d of %d to %s", self.rank, self.world, fx)

    def load(self, path: str):
        """retrieval.py:275-299. Same world size: this rank's shard files only;
        another world size, or a single-GPU save (``<path>.faiss``): the rows
        are re-sharded by global position."""
        path = Path(path)
        data = self._read_pkl(path)
        n = int(data["current_size"])
        saved_world = data.get("world")
        self._reset()
        cfg = data.get("config", {})
        self.metric = cfg.get("metric", self.metric)
        if saved_world == self.world:
            fx, fp = self._shard_files(path, self.rank, self.world)
            vecs, _ = read_flat_index(fx)
            pos = np.load(fp, allow_pickle=False)
            self.shard_sizes = [int(s) for s in data["shard_sizes"]]
        else:
            if saved_world is None:  # a HipFlatIPIndex save: the whole corpus in one file
                full, _ = read_flat_index(path.with_suffix(".faiss"))
            else:
                full = np.zeros((n, self.dimension), np.float32)
                for r in range(saved_world):
                    fx, fp = self._shard_files(path, r, saved_world)
                    v, _ = read_flat_index(fx)
                    full[np.load(fp, allow_pickle=False)] = v
            b, c = self._sh.shard_range(n, self.world, self.rank)
            vecs, pos = full[b:b + c], np.arange(b, b + c, dtype=np.int64)
            self.shard_sizes = [self._sh.shard_range(n, self.world, r)[1] for r in range(self.world)]
        if vecs.shape[1] != self.dimension:
            raise ValueError(f"{path}: dimension {vecs.shape[1]} != {self.dimension}")
        contiguous = pos.size == 0 or bool(np.all(np.diff(pos) == 1))
        self.begin = int(pos[0]) if pos.size else int(sum(self.shard_sizes[:self.rank]))
        self._append_local(torch.from_numpy(vecs).to(self._dev()),  # stored rows: no second renorm
                           None if contiguous else torch.from_numpy(pos))
        self._load_ids(data, n)
        self.current_size = n
        logger.info("Loaded shard %d of %d from %s (%d of %d rows)", self.rank, self.world, path, self.n_local, n)


class _PositionIds:
    """id_map of an index built without ids: position p -> str(p)."""

    def __init__(self, n: int):
        self.n = n

    def __contains__(self, p) -> bool:
        return 0 <= p < self.n

    def __getitem__(self, p) -> str:
        return str(p)


def _sorted_positions(positions, n: int) -> np.ndarray:
    """Ascending unique int32 corpus positions in [0, n) of one exclusion list."""
    a = np.asarray(positions.cpu() if isinstance(positions, torch.Tensor) else positions).reshape(-1)
    if a.size == 0:
        return np.zeros(0, np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError("excluded positions must be integers")
    a = np.unique(a.astype(np.int64, copy=False))
    return a[(a >= 0) & (a < n)].astype(np.int32)


def _mask_words(m, nq: int) -> Optional[np.ndarray]:
    """Per-query 64-bit masks (numpy or tensor, uint64 or int64; None stays None) as
    int64 words [nq] on the host."""
    if m is None:
        return None
    if isinstance(m, torch.Tensor):
        if m.dtype not in (torch.int64, torch.uint64):
            raise TypeError("category masks are 64-bit words (int64 or uint64)")
        m = m.cpu().view(torch.int64).numpy()
    m = np.asarray(m).reshape(-1)
    if m.dtype not in (np.dtype(np.int64), np.dtype(np.uint64)):
        raise TypeError("category masks are 64-bit words (int64 or uint64)")
    if m.shape[0] != nq:
        raise ValueError(f"{m.shape[0]} category masks for {nq} queries")
    return np.ascontiguousarray(m).view(np.int64)


def _mask_tensor(m, nq: int, device) -> Optional[torch.Tensor]:
    """:func:`_mask_words` on ``device`` (a device tensor of the right form is passed on)."""
    if isinstance(m, torch.Tensor) and m.device.type == "cuda" and m.dtype == torch.int64 and m.numel() == nq \
            and m.dim() == 1 and m.is_contiguous():
        return m
    w = _mask_words(m, nq)
    return None if w is None else torch.from_numpy(w.copy()).to(device)


def _per_query(ids, nq: int) -> List:
    """``exclude_ids`` as ``nq`` lists: one flat list of ids serves every query."""
    ids = list(ids)
    if all(isinstance(i, (str, bytes)) or not hasattr(i, "__iter__") for i in ids):
        return [ids] * nq
    if len(ids) != nq:
        raise ValueError(f"exclude_ids holds {len(ids)} lists for {nq} queries")
    return [list(i) for i in ids]


def _exclude_positions(reverse_id_map: Dict[str, int], exclude_ids, nq: int) -> List[np.ndarray]:
    """Per query: the ascending unique positions of the known ids of ``exclude_ids``."""
    out, memo = [], {}
    for ids in _per_query(exclude_ids, nq):
        got = memo.get(id(ids))
        if got is None:
            pos = [reverse_id_map[i] for i in ids if i in reverse_id_map]
            got = memo[id(ids)] = np.unique(np.asarray(pos, dtype=np.int64)).astype(np.int32)
        out.append(got)
    return out


def _lists_from_positions(scores: np.ndarray, pos: np.ndarray, id_map: Dict[int, str], k: int,
                          filter_ids: Optional[List[str]]) -> Tuple[List[List[str]], List[List[float]]]:
    """retrieval.py:176-195: positions -> string ids, -1 padding dropped, the
    filter applied, at most k per query."""
    allowed = set(filter_ids) if filter_ids is not None else None
    batch_ids, batch_scores = [], []
    for i in range(pos.shape[0]):
        item_ids, item_scores = [], []
        for j in range(pos.shape[1]):
            p = int(pos[i, j])
            if p >= 0 and p in id_map:
                item_id = id_map[p]
                if allowed is None or item_id in allowed:
                    item_ids.append(item_id)
                    item_scores.append(float(scores[i, j]))
                    if len(item_ids) >= k:
                        break
        batch_ids.append(item_ids)
        batch_scores.append(item_scores)
    return batch_ids, batch_scores


_IVF_FACTORY = "IVF1024,Flat"   # the reference's default (retrieval.py:60)
IVF_MIN_ITEMS = 1024            # below it the reference builds Flat (retrieval.py:90-93)
_ASSIGN_CHUNK = 1 << 20         # rows per nearest-centroid call


def _parse_ivf_factory(factory: str) -> int:
    """``"IVF<nlist>,Flat"`` -> nlist; anything else raises."""
    s = str(factory)
    head, _, tail = s.partition(",")
    if not head.startswith("IVF") or tail != "Flat" or not head[3:].isdigit() or int(head[3:]) < 1:
        raise ValueError(f"index_factory {factory!r}: HipIVFFlatIndex serves 'IVF<nlist>,Flat' "
                         "(every other factory: HipFlatIPIndex, exact)")
    return int(head[3:])


class HipIVFFlatIndex(_HbmIndex):
    """IVF-Flat index resident in HBM: the reference's DEFAULT configuration,
    ``faiss.index_factory(d, "IVF1024,Flat")`` searched with ``nprobe = 20``
    (retrieval.py:60-62, 101-133). k-means lists over the corpus, a coarse
    search over the centroids, then an exact scan of the probed lists only
    (``rt_ivf_topk``): a search reads about nprobe / nlist of the rows.

    Scores are the Flat index's, bit for bit (the same sequential fmaf chain),
    and results keep its order — (score desc, original position asc), -1 pads —
    so a search with ``nprobe == nlist`` IS the Flat search, and one with fewer
    probes is the Flat search restricted to the probed lists. Faiss's own
    k-means cannot be reproduced bit for bit (random subsampling and
    initialisation); this one is deterministic: the same data and ``seed`` give
    the same index, bit for bit.

    Config keys: ``dimension``; ``metric`` ("cosine" or "inner_product"; the L2
    metric raises — use :class:`HipFlatIPIndex`); ``index_factory``
    (``"IVF<nlist>,Flat"``, default ``"IVF1024,Flat"``; anything else raises);
    ``nprobe`` (default 20, clamped to nlist at search; a plain attribute that
    may be changed between searches, as with Faiss; at most 128 lists are
    probed per search); ``storage_dtype``, ``device``; ``train_iters`` (10);
    ``max_points_per_centroid`` (256: training subsamples to that many rows per
    list); ``seed`` (1234); ``online_max_batch`` (as :class:`HipFlatIPIndex`:
    small calls go through the resident :class:`OnlineIVFSearcher`, with
    ``exclude_ids`` too: its scan reads the lists, ``rt_ivf_topk_lists``; measured
    0.14-0.25 ms against 0.21-0.31 ms through a bitmap at 1M rows).
    ``batch_min_queries`` (default ``None`` = off; an integer >= 1): calls of
    ``search_tensors`` — and of everything above it: ``search`` with
    ``exclude_ids`` / ``filter_ids``, ``RetrievalEngine.retrieve`` — with at least
    that many queries take the list-major scan (``rt_ivf_topk_batch``: one pass
    over a list for all queries of a tile that probe it) instead of one scan block
    per (query, probed list); the results are the same bit for bit. Calls at or
    below ``online_max_batch`` keep the resident searcher, the Flat fallback
    ignores the key, save / load keep it with the config. Measured at 1M x 128,
    nprobe 20, k 100 ("IVF batch search"): the crossover is 4,096
    queries per call — 0.90x (float16) and 0.79x (float32) the per-query path's
    time there, slower below it (1.03-1.05x at 1,024, about 2x at 16-256) — so
    4096 is the recommended value.
    ``mutable: True`` raises and names :class:`HipMutableIVFFlatIndex` (index
    type ``hip_ivf_mutable``), whose lists change in place; on this class
    ``update`` and ``remove`` only warn, as the reference's do. k <= 128 per
    search (2k <= 128 with ``filter_ids``).

    Below 1,024 items, or below nlist, ``build`` logs the reference's message
    and everything is delegated to an inner :class:`HipFlatIPIndex`.

    Measured ("IVF-Flat"; 1M x 128, k = 100, nlist = 1024,
    resident searchers alternating call by call): at nprobe = 20 the call is
    1.31x the exact online search's for one float16 query (slower: four chained
    launches against two, both latency-bound), 0.87x for 8 float16 queries,
    0.89x / 0.81x for 1 / 8 float32 queries; recall@100 0.998. Recommended from
    about 1M rows for float32 storage or 8-query calls and, extrapolated, from
    1.5-2M rows for single float16 queries; below that ``HipFlatIPIndex`` with
    ``online_max_batch`` is as fast and exact.

    ``categories``: as :class:`HipFlatIPIndex`. The tags are kept by ORIGINAL
    position (the lists know nothing of them); a filtered search is exact over
    the eligible rows of the PROBED lists — k results whenever k eligible rows
    exist among them, as a filtered Faiss IVF search — not over the corpus: a
    narrow filter may need a larger ``nprobe``. The resident path tests the tags
    in the probed-list scan (``rt_ivf_topk_tags``); larger calls, the
    ``batch_min_queries`` route included, take ``rt_tag_filter_bitmap``.
    Measured ("Category filters"; 1M x 128, k = 100, nlist 1024, nprobe 20, nq 1 and
    8, float16 and float32, 50 / 10 / 1 % eligible; p50 of the resident call in us): 120-164
    without a filter, 85-150 with it (-48 to -8 us), against 158-212 through the bitmap route.
    """

    _searcher_takes_exclude = True   # OnlineIVFSearcher: rt_ivf_topk_lists
    _lists_mutable = False           # HipMutableIVFFlatIndex: lists with slack, changed in place

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(dict(config or {}))
        if self.config.get("mutable", False) and not self._lists_mutable:
            raise ValueError("HipIVFFlatIndex is not mutable: its lists are stored without slack; "
                             "HipMutableIVFFlatIndex (index type 'hip_ivf_mutable') updates, adds and removes "
                             "in place (for a Flat index: HipFlatIPIndex with mutable=True)")
        self.mutable = self._lists_mutable
        self.index_factory = self.config.get("index_factory", _IVF_FACTORY)
        self.nlist = _parse_ivf_factory(self.index_factory)
        self.nprobe = int(self.config.get("nprobe", 20))
        self.train_iters = int(self.config.get("train_iters", 10))
        self.max_points_per_centroid = int(self.config.get("max_points_per_centroid", 256))
        self.seed = int(self.config.get("seed", 1234))
        self._init_online()
        self._init_batch()
        self._flat: Optional[HipFlatIPIndex] = None   # the Flat fallback of a small corpus
        self.index: Optional[torch.Tensor] = None     # [n, d] storage dtype, list-contiguous
        self.centroids: Optional[torch.Tensor] = None     # [nlist, d] fp32
        self.list_offsets: Optional[torch.Tensor] = None  # [nlist + 1] int64
        self.row_pos: Optional[torch.Tensor] = None       # [n] int32: original position of a stored row
        self.assign: Optional[torch.Tensor] = None        # [n] int64: list of an original position
        self.max_list_rows = 0

    def _check_metric(self):
        if self._l2:
            raise ValueError(f"metric {self.metric!r}: HipIVFFlatIndex serves 'cosine' and 'inner_product'; "
                             "the L2 metric (IndexFlatL2) is HipFlatIPIndex")

    # -- helpers -----------------------------------------------------------
    def _init_batch(self):
        """The ``batch_min_queries`` option: None (off) or the smallest batch that takes
        the list-major scan."""
        v = self.config.get("batch_min_queries")
        self.batch_min_queries = None if v is None else int(v)
        if self.batch_min_queries is not None and self.batch_min_queries < 1:
            raise ValueError(f"batch_min_queries={self.batch_min_queries}: None (off) or >= 1")

    def _flat_config(self) -> Dict[str, Any]:
        cfg = {k: v for k, v in self.config.items()
               if k in ("dimension", "metric", "storage_dtype", "device", "online_max_batch", "categories")}
        cfg["index_factory"] = "Flat"
        return cfg

    def _scan_operands(self) -> Dict[str, Any]:
        """What ``kernels.ivf_topk`` / ``kernels.ivf_topk_batch`` take beyond the lists of
        this class (none)."""
        return {}

    def _live_assign(self) -> torch.Tensor:
        """The list of every position in [0, current_size)."""
        return self.assign

    def _assign_rows(self, rows: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        """Nearest centroid of every fp32 row by inner product, the lowest centroid
        id winning ties (rt_flatip_topk, k = 1: rows as queries, centroids as items)."""
        out = torch.empty(rows.shape[0], dtype=torch.int64, device=rows.device)
        for a in range(0, rows.shape[0], _ASSIGN_CHUNK):
            _, ids = kernels.flatip_topk(rows[a:a + _ASSIGN_CHUNK], centroids, 1)
            out[a:a + _ASSIGN_CHUNK] = ids.view(-1)
        return out

    def _group(self, assign: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(order, offsets, counts): the stable sort of the assignments (original order
        kept within a list) and the lists' CSR offsets."""
        order = torch.sort(assign, stable=True).indices
        counts = torch.bincount(assign, minlength=self.nlist)
        offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=assign.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return order, offsets, counts

    def _train(self, rows: torch.Tensor) -> torch.Tensor:
        """``train_iters`` Lloyd steps over all rows, or over a seeded subsample of
        ``max_points_per_centroid x nlist`` of them in ascending position order;
        the initial centroids are the rows at the first nlist entries of the
        same permutation. An empty list keeps its centroid."""
        n = rows.shape[0]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed))
        centroids = rows[perm[: self.nlist].to(rows.device)].contiguous()
        n_train = self.max_points_per_centroid * self.nlist
        train = rows
        if n > n_train:
            sub = torch.sort(perm[:n_train]).values.to(rows.device)
            train = kernels.gather_rows(rows, sub)
        for _ in range(self.train_iters):
            order, offsets, _ = self._group(self._assign_rows(train, centroids))
            grouped = kernels.gather_rows(train, order)
            centroids = kernels.segment_mean(grouped, offsets, centroids, normalize=self.metric == "cosine")
        return centroids

    def _regroup(self, src: torch.Tensor, src_index: Optional[torch.Tensor], assign: torch.Tensor):
        """Store the rows list-contiguous: stored row i is ``src[src_index[order[i]]]``
        (``src_index`` None: ``src`` is in original order) — one gather."""
        order, offsets, counts = self._group(assign)
        self.index = kernels.gather_rows(src, order if src_index is None else src_index[order])
        self.row_pos = order.to(torch.int32)
        self._inv_row_pos = None   # the re-rank's inverse of row_pos: made again when next needed
        self.list_offsets = offsets
        self.assign = assign
        self.max_list_rows = int(counts.max().item()) if assign.numel() else 0
        self.current_size = int(assign.numel())

    def _sync_flat(self):
        """Mirror the inner Flat index's public state (the fallback of a small corpus)."""
        f = self._flat
        self.id_map, self.reverse_id_map, self._ids = f.id_map, f.reverse_id_map, f._ids
        self.current_size = f.current_size
        self.index = f.index
        self._tags = f._tags
        self._generation += 1

    # -- IndexBase ---------------------------------------------------------
    def build(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:70-139: normalise (cosine), train the coarse quantiser
        (``index.train``), add every row to its list (``index.add``).
        ``item_categories`` as :meth:`HipFlatIPIndex.build` takes it; the tags are
        kept by ORIGINAL position, so the lists know nothing of them."""
        start = time.time()
        n = len(embeddings)
        self._online = None
        tags = self._item_tags(item_categories, n)
        if n < IVF_MIN_ITEMS or n < self.nlist:
            logger.info("Dataset too small (%d) for IVF, using Flat index", n)
            self._flat = HipFlatIPIndex(self._flat_config())
            self._flat.build(embeddings, ids, item_categories=item_categories)
            self.centroids = self.list_offsets = self.row_pos = self.assign = None
            self._sync_flat()
            return
        self._flat = None
        rows = self._prepare(embeddings)
        self.centroids = self._train(rows)
        assign = self._assign_rows(rows, self.centroids)
        self._regroup(rows.to(self.storage_dtype), None, assign)
        self._tags = None
        self._tags_store(0, tags)
        self._reset_ids()
        self._record_ids(0, ids, max(n, len(ids)))   # ids past the rows stay in _ids, as in the Flat index
        self._generation += 1
        logger.info("Index built in %.2f seconds", time.time() - start)

    def online_searcher(self, max_batch: int = 8, max_exclude: int = 8192) -> "OnlineSearcher":
        """The resident searcher for calls of at most ``max_batch`` (1..8) queries and
        k <= 128: an :class:`OnlineIVFSearcher` (the Flat fallback: an
        :class:`OnlineSearcher` over the inner Flat index); ``max_exclude``: the
        exclusion-list entries one call may carry through its resident buffers."""
        if self._flat is not None:
            return self._flat.online_searcher(max_batch, max_exclude)
        return OnlineIVFSearcher(self, max_batch, max_exclude)

    def _n_probe(self, nprobe: Optional[int] = None) -> int:
        np_ = min(int(self.nprobe if nprobe is None else nprobe), self.nlist)
        if not 1 <= np_ <= kernels.IVF_MAX_NPROBE:
            raise ValueError(f"nprobe={np_}: the MI355X IVF index probes 1..{kernels.IVF_MAX_NPROBE} lists per search")
        return np_

    def search_tensors(self, query_embeddings: Array, k: int, exclude_bits: Optional[torch.Tensor] = None,
                       nprobe: Optional[int] = None, tag_filter=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-level search: (scores [nq, k], original positions [nq, k]) with
        (-FLT_MAX, -1) padding, like the Flat index. The coarse search runs on the
        fp32 queries, before the storage cast. ``tag_filter=(any_of, none_of)``: as
        :meth:`HipFlatIPIndex.search_tensors` (a bitmap by original position, for
        the list-major batch scan too); exact over the PROBED lists."""
        if self.index is None:
            raise ValueError("Index not built yet")
        if self._flat is not None:
            return self._flat.search_tensors(query_embeddings, k, exclude_bits=exclude_bits, tag_filter=tag_filter)
        if not 1 <= k <= kernels.IVF_MAX_K:
            raise ValueError(f"k={k}: the MI355X IVF index returns 1..{kernels.IVF_MAX_K} results per query")
        np_ = self._n_probe(nprobe)
        q32 = self._prepare(query_embeddings)
        exclude_bits = self._filter_bits(tag_filter, q32.shape[0], exclude_bits)
        if q32.shape[0] <= kernels.ONLINE_MAX_NQ:
            _, probes = kernels.flatip_topk_online(q32, self.centroids, np_)
        else:
            _, probes = kernels.flatip_topk(q32, self.centroids, np_)
        # a batch of batch_min_queries or more: one pass over a list for all queries that
        # probe it (rt_ivf_topk_batch); the same results, bit for bit
        batch = self.batch_min_queries is not None and q32.shape[0] >= self.batch_min_queries
        scan = kernels.ivf_topk_batch if batch else kernels.ivf_topk
        return scan(q32.to(self.storage_dtype), self.index, self.list_offsets, self.row_pos, probes,
                    self.max_list_rows, k, exclude_bits=exclude_bits, **self._scan_operands())

    def _mmr_operands(self):
        """The lists' rows and the stored row of every position: the inverse of
        ``row_pos``, one torch scatter per generation, made at the first re-ranked
        search and dropped with the generation."""
        if self._flat is not None:
            return self._flat._mmr_operands()
        made = getattr(self, "_inv_row_pos", None)
        if made is None or made[0] != self._generation:
            inv = torch.full((self.current_size,), -1, dtype=torch.int32, device=self.row_pos.device)
            inv[self.row_pos.long()] = torch.arange(self.row_pos.numel(), dtype=torch.int32, device=inv.device)
            made = self._inv_row_pos = (self._generation, inv)
        return self.index, made[1], self.current_size

    def search(self, query_embeddings: Array, k: int = 10, filter_ids: Optional[List[str]] = None,
               exclude_ids=None, filter_categories=None, exclude_categories=None,
               mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None
               ) -> Tuple[List[List[str]], List[List[float]]]:
        """retrieval.py:141-197, as :meth:`HipFlatIPIndex.search`: the 2k over-fetch
        for ``filter_ids``, exact ``exclude_ids`` in the search (over the probed
        lists). With ``online_max_batch`` a small call with ``exclude_ids`` stays on
        the resident searcher, whose scan reads the lists (``rt_ivf_topk_lists``);
        the other calls mask through a bitmap. ``filter_categories`` /
        ``exclude_categories``: as :meth:`HipFlatIPIndex.search`, exact over the
        PROBED lists (k results whenever k eligible rows exist among them), as a
        filtered Faiss IVF search is — not over the corpus. ``mmr_lambda`` /
        ``mmr_candidates``: as :meth:`HipFlatIPIndex.search`; the candidates are the
        top ``mmr_candidates`` of the probed lists, and the re-rank depends on the
        candidates and their stored values only, so with every list probed the
        lists are the Flat index's."""
        cats = dict(filter_categories=filter_categories, exclude_categories=exclude_categories)
        if mmr_lambda is not None or mmr_candidates is not None:
            cats.update(mmr_lambda=mmr_lambda, mmr_candidates=mmr_candidates)
        if self.index is not None and self._flat is not None:
            return self._flat.search(query_embeddings, k, filter_ids, exclude_ids=exclude_ids, **cats)
        return super().search(query_embeddings, k, filter_ids, exclude_ids=exclude_ids, **cats)

    def add(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:199-226. The new rows are assigned to the existing centroids
        (no retraining), then every list is regrouped by a stable sort of all
        assignments and one gather: O(n) per call in the size of the index, not
        in the size of the batch — batch the additions
        (:class:`HipMutableIVFFlatIndex` adds in O(batch))."""
        if self.index is None:
            raise ValueError("Index not built yet")
        if self._flat is not None:
            self._flat.add(embeddings, ids, item_categories=item_categories)
            self._sync_flat()
            return
        rows = self._prepare(embeddings)
        n_old, m = self.current_size, rows.shape[0]
        tags = self._item_tags(item_categories, m)
        dev = rows.device
        inv = torch.empty(n_old, dtype=torch.int64, device=dev)
        inv[self.row_pos.long()] = torch.arange(n_old, dtype=torch.int64, device=dev)
        src_index = torch.cat([inv, torch.arange(n_old, n_old + m, dtype=torch.int64, device=dev)])
        assign = torch.cat([self.assign, self._assign_rows(rows, self.centroids)])
        src = torch.cat([self.index, rows.to(self.storage_dtype)])
        with self._searcher_lock():
            self._regroup(src, src_index, assign)
            self._tags_store(n_old, tags)
            self._record_ids(n_old, ids, max(m, len(ids)))
            self._generation += 1
        logger.info("Added %d items to index. Total size: %d", m, self.current_size)

    def update(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:228-237: a no-op with a warning, like the reference
        (``set_item_categories`` changes tags alone)."""
        logger.warning("IVF index doesn't support direct updates. Consider periodic rebuilds.")

    def remove(self, ids: List[str]):
        """retrieval.py:239-246: a no-op with a warning, like the reference."""
        logger.warning("IVF index doesn't support removal. Consider periodic rebuilds.")
        return None

    def vectors(self) -> np.ndarray:
        """The stored rows in original order (fp32)."""
        if self._flat is not None:
            return self._flat.vectors()
        if self.index is None:
            return np.zeros((0, self.dimension), np.float32)
        out = torch.empty_like(self.index)
        out[self.row_pos.long()] = self.index
        return out.float().cpu().numpy()

    def save(self, path: str):
        """``<path>.faiss`` (the rows in original order, IndexFlatIP layout) and
        ``<path>.pkl`` (id maps) as the Flat index writes them, plus
        ``<path>.ivf.npz``: centroids, assignments, config and seed."""
        if self.index is None:
            raise ValueError("No index to save")
        path = Path(path)
        if self._flat is not None:
            self._flat.save(str(path))   # its .tags.npz too
            ivf = path.with_suffix(".ivf.npz")
            if ivf.exists():
                ivf.unlink()   # a stale file of an earlier IVF save under this name
            return
        path.parent.mkdir(parents=True, exist_ok=True)
        write_flat_index(path.with_suffix(".faiss"), self.vectors(), True)
        self._save_ids(path)
        cfg = {k: v for k, v in self.config.items() if isinstance(v, (str, int, float, bool, type(None)))}
        np.savez(path.with_suffix(".ivf.npz"), centroids=self.centroids.cpu().numpy(),
                 assign=self._live_assign().cpu().numpy(), config=np.array(json.dumps(cfg)), seed=np.int64(self.seed),
                 nlist=np.int64(self.nlist))
        self._save_tags(path)
        logger.info("Saved index to %s", path)

    def load(self, path: str):
        """retrieval.py:275-299. A loaded index answers bit-identically: the rows are
        regrouped by the saved assignments, nothing is trained again."""
        path = Path(path)
        self._online = None
        ivf = path.with_suffix(".ivf.npz")
        if not ivf.exists():   # saved by the Flat fallback (or by HipFlatIPIndex)
            self._flat = HipFlatIPIndex(self._flat_config())
            self._flat.load(str(path))
            self.dimension, self.metric = self._flat.dimension, self._flat.metric
            self.centroids = self.list_offsets = self.row_pos = self.assign = None
            self.categories, self._cat_bit = self._flat.categories, self._flat._cat_bit
            self._sync_flat()
            return
        vecs, _ip = read_flat_index(path.with_suffix(".faiss"))
        data = self._read_pkl(path)
        with np.load(ivf) as z:
            centroids, assign = z["centroids"], z["assign"]
            self.seed, self.nlist = int(z["seed"]), int(z["nlist"])
        self._flat = None
        self.config = dict(data.get("config", self.config))
        self.metric = self.config.get("metric", self.metric)
        self._init_batch()
        self.dimension = vecs.shape[1]
        self.index_factory = f"IVF{self.nlist},Flat"
        dev = self._dev()
        self.centroids = torch.from_numpy(centroids).to(dev)
        self._regroup(torch.from_numpy(vecs).to(dev).to(self.storage_dtype), None, torch.from_numpy(assign).to(dev))
        self._load_ids(data, self.current_size)
        self._load_tags(path)
        self._generation += 1
        logger.info("Loaded index from %s with %d items", path, self.current_size)


class OnlineIVFSearcher(OnlineSearcher):
    """:class:`OnlineSearcher` over one :class:`HipIVFFlatIndex`
    (``index.online_searcher(max_batch)``): the same pinned buffers, one graph
    replay and one synchronise per call; the captured chain is ``l2_renorm``
    (cosine) -> coarse ``rt_flatip_topk_online`` over the fp32 centroids with
    k = nprobe -> storage-dtype cast -> ``rt_ivf_topk`` — the arithmetic of
    ``HipIVFFlatIndex.search_tensors`` in the same order. One graph per
    (nq, k, nprobe): ``index.nprobe`` is read at every call. Generation
    invalidation as the base class (``build`` / ``add`` / ``load``).

    Exclusion lists (``search(q, k, exclude=...)``) are staged and uploaded as in
    the base class and read by the probed-list scan (``rt_ivf_topk_lists``: a
    membership test per candidate row, in ORIGINAL positions): graphs with
    lists are keyed (nq, k, nprobe, True), one for every list length up to
    ``max_exclude`` entries per call. A call with more takes the bitmap path
    through ``search_tensors`` and returns fresh arrays, as in the base class."""

    def __init__(self, index: "HipIVFFlatIndex", max_batch: int = 8, max_exclude: int = 8192):
        if not isinstance(index, HipIVFFlatIndex) or index._flat is not None or index.index is None:
            raise ValueError("OnlineIVFSearcher serves a built HipIVFFlatIndex that holds lists "
                             "(a small corpus falls back to Flat: index.online_searcher() returns its searcher)")
        super().__init__(index, max_batch, max_exclude)
        dev, mb = index._dev(), self.max_batch
        # workspace sizing: both searches write [mb][<= 128][<= 512 lists] 8-byte keys at most —
        # the base class's bound; the coarse search gets a workspace of its own
        self._ws_coarse = torch.empty(mb * self.MAX_K * 512 * 8, dtype=torch.uint8, device=dev)
        self._d_cs = torch.empty(mb * kernels.IVF_MAX_NPROBE, dtype=torch.float32, device=dev)
        self._d_probes = torch.empty(mb * kernels.IVF_MAX_NPROBE, dtype=torch.int64, device=dev)
        self._nprobe = 0
        self._lists = None
        self._scan_operands: Dict[str, Any] = {}

    def _graph_key(self, nq: int, k: int, lists: bool) -> tuple:
        return (nq, k, self._nprobe, True) if lists else (nq, k, self._nprobe)

    def _revalidate(self) -> bool:
        idx = self.index
        self._nprobe = idx._n_probe() if idx._flat is None else 0   # read at every call
        if self._generation == idx._generation:
            return False
        self._graphs.clear()
        if idx._flat is not None or idx.dimension != self._h_q.shape[1] or idx.storage_dtype != self._d_q.dtype:
            raise ValueError("the index changed its dimension, storage dtype or fell back to Flat since this "
                             "searcher was made: obtain a new one (index.online_searcher)")
        self._rows = idx.index
        self._item_tags = idx._tags
        self._lists = (idx.list_offsets, idx.row_pos, idx.centroids, idx.max_list_rows)
        self._scan_operands = idx._scan_operands()   # a mutable index: list_len and n_pos, fixed per generation
        self._mmr_ops = None
        self._generation = idx._generation
        return True

    def _device_chain(self, nq: int, k: int, sources=None, tags: bool = False):
        """As the base class's, over the lists (``tags``: ``rt_ivf_topk_tags``, the
        resident tags indexed by ORIGINAL position): ``l2_renorm`` (cosine) -> coarse search
        -> storage-dtype cast -> ``rt_ivf_topk`` (``sources``: ``rt_ivf_topk_lists`` with
        these exclusion sources, positions in ORIGINAL order); over a
        :class:`HipMutableIVFFlatIndex` their ``_lens`` forms, which read ``list_len``."""
        n, np_ = nq * k, self._nprobe
        offsets, row_pos, centroids, max_list_rows = self._lists
        q32 = self._d_q32[:nq]
        if self.index.metric == "cosine":
            kernels.l2_renorm_(q32)
        probes = self._d_probes[:nq * np_].view(nq, np_)
        kernels.flatip_topk_online(q32, centroids, np_, out=(self._d_cs[:nq * np_].view(nq, np_), probes),
                                   workspace_buf=self._ws_coarse)
        q = self._d_q[:nq]
        if q.data_ptr() != q32.data_ptr():
            q.copy_(q32)
        kernels.ivf_topk(q, self._rows, offsets, row_pos, probes, max_list_rows, k,
                         out=(self._d_s[:n].view(nq, k), self._d_p[:n].view(nq, k)), workspace_buf=self._ws,
                         exclude_lists=sources or None, tag_filter=self._tag_filter(nq) if tags else None,
                         **self._scan_operands)


class HipMutableIVFFlatIndex(HipIVFFlatIndex):
    """:class:`HipIVFFlatIndex` whose lists change where they lie: ``update`` is
    an upsert, ``add`` costs O(batch) and ``remove`` withdraws items — the
    streaming ``item_update`` path (``RetrievalEngine.update_index``) on the
    reference's default ``"IVF1024,Flat"`` index. Index type ``hip_ivf_mutable``;
    ``.mutable`` is True. Searches, scores, result order, ``exclude_ids``, the
    resident :class:`OnlineIVFSearcher` and :class:`~rtrec_amd.serving.online.
    OnlineRecommender` are the base class's: the scan is the same kernel, told
    each list's live length (``rt_ivf_topk_lens``).

    Layout: list l owns a fixed range of stored rows — its capacity, ``len +
    max(min_slack_rows, ceil(len x list_slack))`` at every (re)group — of which
    the first ``list_len[l]`` are live; ``row_pos`` is -1 in the rest. Config
    keys beyond the base class's: ``list_slack`` (default 0.25) and
    ``min_slack_rows`` (default 32). Both defaults are policy choices, not
    measured: more slack means fewer regroups and more HBM. The device holds
    the lists, ``list_len``, ``pos_slot`` (the stored row of a position) and
    ``assign``; the host holds the id maps, the size and the capacities only.

    ``update(embeddings, ids)``: rows are prepared and assigned to the existing
    centroids (no retraining); the last occurrence of an id given twice wins.
    A known id's row is overwritten in place, or moved to its new nearest list
    (``rt_ivf_lists_update``, one call per batch); its position does not
    change, no pointer, size or ``max_list_rows`` changes, so the generation is
    NOT bumped and captured serving graphs stay valid and read the new row at
    their next replay. Unknown ids are appended as by ``add``, in call order.

    ``add``: the new rows take the positions ``current_size ...`` and join their
    lists through the same kernel call; the generation is bumped (the number of
    positions is a captured host argument). An id already stored is stored
    again, and ``reverse_id_map`` then names the last row, as on the Flat index.

    ``remove(ids)``: every row stored under one of the ids leaves its list, and
    positions are made dense again by this rule (NOT the Flat index's
    shift-down): with R the removed positions and n' = n - |R|, the surviving
    positions >= n' take, in ascending order, the removed positions < n', in
    ascending order; no other item changes position. Equal scores tie by
    position, so after a ``remove`` ties resolve by the rule's positions, not
    by those of an index rebuilt on the surviving items. The id maps are
    updated in O(|R|), the generation is bumped (``OnlineRecommender`` remaps
    its seen lists); returns the number of rows removed, unknown ids are ignored.

    A batch that would overflow a list's capacity changes nothing on the device;
    the index then regroups every list once with fresh slack, the batch
    included — the O(n) path of the base class's ``add``, amortised — bumps the
    generation and logs at info level.

    ``save`` writes the live rows in position order in the base class's three
    files; a loaded index answers bit-identically (results never depend on the
    storage order). Below 1,024 items or below nlist everything is delegated to
    an inner :class:`HipFlatIPIndex` with ``mutable: True``.
    """

    _lists_mutable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.list_slack = float(self.config.get("list_slack", 0.25))
        self.min_slack_rows = int(self.config.get("min_slack_rows", 32))
        if self.list_slack < 0 or self.min_slack_rows < 0:
            raise ValueError(f"list_slack={self.list_slack}, min_slack_rows={self.min_slack_rows}: both >= 0")
        self.list_len: Optional[torch.Tensor] = None    # [nlist] int64: live rows of a list
        self.pos_slot: Optional[torch.Tensor] = None    # [capacity] int32: stored row of a position, -1 none
        self.capacity = 0                               # stored rows in all: len(index), len(row_pos), ...

    # -- helpers -----------------------------------------------------------
    def _flat_config(self) -> Dict[str, Any]:
        cfg = super()._flat_config()
        cfg["mutable"] = True
        return cfg

    def _scan_operands(self) -> Dict[str, Any]:
        return {"list_len": self.list_len, "n_pos": self.current_size}

    def _live_assign(self) -> torch.Tensor:
        return self.assign[: self.current_size]

    def _mmr_operands(self):
        if self._flat is not None:
            return self._flat._mmr_operands()
        # the resident pos_slot: an in-place update rewrites rows and slots where they lie
        return self.index, self.pos_slot, self.current_size

    def _regroup(self, src: torch.Tensor, src_index: Optional[torch.Tensor], assign: torch.Tensor):
        """The base class's regroup into lists with slack: position p (``assign[p]``
        >= 0) is stored from ``src[src_index[p]]``, original order kept within a
        list; every array is sized to the new total capacity."""
        dev, n = assign.device, int(assign.numel())
        live = torch.nonzero(assign >= 0).view(-1)
        a = assign[live]
        order = live[torch.sort(a, stable=True).indices]       # positions, list by list
        counts = torch.bincount(a, minlength=self.nlist)
        slack = torch.clamp(torch.ceil(counts.double() * self.list_slack).long(), min=self.min_slack_rows)
        caps = counts + slack
        offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(caps, 0)
        starts = torch.zeros(self.nlist, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(counts, 0)[:-1]
        lists = assign[order]
        slots = offsets[lists] + (torch.arange(order.numel(), dtype=torch.int64, device=dev) - starts[lists])
        total, max_cap = (int(v) for v in torch.stack([offsets[-1], caps.max()]).tolist())   # the regroup's one read
        total = max(total, n)   # pos_slot / assign hold every position
        src_of_slot = torch.full((total,), -1, dtype=torch.int64, device=dev)
        src_of_slot[slots] = order if src_index is None else src_index[order]
        self.index = kernels.gather_rows(src, src_of_slot)      # an empty slot: a zero row
        self.row_pos = torch.full((total,), -1, dtype=torch.int32, device=dev)
        self.row_pos[slots] = order.to(torch.int32)
        self.pos_slot = torch.full((total,), -1, dtype=torch.int32, device=dev)
        self.pos_slot[order] = slots.to(torch.int32)
        self.assign = torch.full((total,), -1, dtype=torch.int64, device=dev)
        self.assign[:n] = assign
        self.list_offsets, self.list_len = offsets, counts
        self.capacity, self.max_list_rows = total, max_cap
        self.current_size = n

    def _mutate(self, positions: torch.Tensor, new_list: torch.Tensor, new_rows: torch.Tensor, n_pos: int):
        """Apply one batch (``rt_ivf_lists_update``) under the searcher lock; ``n_pos``:
        the positions in use after it. True when the lists were regrouped instead
        (a position past the capacity, or a list that would overflow)."""
        if n_pos <= self.capacity:
            status = kernels.ivf_lists_update(self.index, self.list_offsets, self.list_len, self.row_pos,
                                              self.pos_slot, self.assign, positions, new_list, new_rows)
            overflow, refused = status.tolist()   # the call's one read: 8 bytes
            if refused:
                raise RuntimeError(f"rt_ivf_lists_update refused {refused} operations: the index state is inconsistent")
            if not overflow:
                return False
            logger.info("%d lists would overflow their capacity: regrouping %d rows with fresh slack", overflow, n_pos)
        else:
            logger.info("%d positions exceed the capacity of %d rows: regrouping with fresh slack", n_pos,
                        self.capacity)
        n_old, dev = min(self.current_size, n_pos), positions.device
        assign = torch.full((n_pos,), -1, dtype=torch.int64, device=dev)
        assign[:n_old] = self.assign[:n_old]
        src_index = torch.zeros(n_pos, dtype=torch.int64, device=dev)
        src_index[:n_old] = self.pos_slot[:n_old].long().clamp_(min=0)
        assign[positions] = new_list
        src_index[positions] = self.capacity + torch.arange(positions.numel(), dtype=torch.int64, device=dev)
        self._regroup(torch.cat([self.index, new_rows]), src_index, assign)
        self._generation += 1
        return True

    # -- IndexBase ---------------------------------------------------------
    def add(self, embeddings: Array, ids: List[str], item_categories=None):
        """retrieval.py:199-226 in O(batch): the new rows are assigned to the existing
        centroids and join their lists in place (see the class docstring)."""
        if self.index is None:
            raise ValueError("Index not built yet")
        if self._flat is not None:
            self._flat.add(embeddings, ids, item_categories=item_categories)
            self._sync_flat()
            return
        rows = self._prepare(embeddings)
        self._append(rows, ids, self._item_tags(item_categories, rows.shape[0]))

    def _append(self, rows: torch.Tensor, ids: List[str], tags: Optional[np.ndarray] = None):
        n_old, m = self.current_size, rows.shape[0]
        positions = torch.arange(n_old, n_old + m, dtype=torch.int64, device=rows.device)
        new_list = self._assign_rows(rows, self.centroids) if m else positions
        with self._searcher_lock():
            if m:
                self._mutate(positions, new_list, rows.to(self.storage_dtype), n_old + m)
            self._tags_store(n_old, np.zeros(m, np.uint64) if tags is None else tags)
            self.current_size = n_old + m
            self._record_ids(n_old, ids, max(m, len(ids)))
            self._generation += 1
        logger.info("Added %d items to index. Total size: %d", m, self.current_size)

    def update(self, embeddings: Array, ids: List[str], item_categories=None):
        """An upsert (see the class docstring): known ids in place, without a
        generation bump; unknown ids appended as by ``add``. ``item_categories``:
        None keeps the tags of known ids; given, they are overwritten in place."""
        if self.index is None:
            raise ValueError("Index not built yet")
        if self._flat is not None:
            self._flat.update(embeddings, ids, item_categories=item_categories)
            self._sync_flat()
            return
        ids = list(ids)
        rows = self._prepare(embeddings)
        if rows.shape[0] != len(ids):
            raise ValueError(f"{rows.shape[0]} embeddings for {len(ids)} ids")
        tags = None if item_categories is None else self._item_tags(item_categories, len(ids))
        known: Dict[str, int] = {}     # id -> its last row in the call (positions stay unique)
        unknown: Dict[str, int] = {}   # in order of first appearance, the last row wins too
        for i, item_id in enumerate(ids):
            (known if item_id in self.reverse_id_map else unknown)[item_id] = i
        if known:
            take = torch.tensor(list(known.values()), dtype=torch.int64, device=rows.device)
            pos = torch.tensor([self.reverse_id_map[i] for i in known], dtype=torch.int64, device=rows.device)
            new = rows[take]
            new_list = self._assign_rows(new, self.centroids)
            with self._searcher_lock():   # row and tags under one acquisition: a search sees both or neither
                self._mutate(pos, new_list, new.to(self.storage_dtype), self.current_size)
                if tags is not None:
                    self._tags_write([self.reverse_id_map[i] for i in known], tags[list(known.values())])
        if unknown:
            take = torch.tensor(list(unknown.values()), dtype=torch.int64, device=rows.device)
            self._append(rows[take], list(unknown), None if tags is None else tags[list(unknown.values())])
        logger.info("Updated %d items in place, appended %d. Total size: %d", len(known), len(unknown),
                    self.current_size)

    def remove(self, ids: List[str]) -> Optional[int]:
        """Withdraw every row stored under one of ``ids`` and renumber by the rule of
        the class docstring. Returns the number of rows removed."""
        if self.index is None:
            raise ValueError("Index not built yet")
        if self._flat is not None:
            removed = self._flat.remove(ids)
            self._sync_flat()
            return removed
        hit = {i for i in ids if i in self.reverse_id_map}
        if not hit:
            return 0
        n = self.current_size
        gone = {self.reverse_id_map[i] for i in hit}
        if len(self.id_map) != len(self.reverse_id_map):
            # an id stored more than once through add: every one of its rows goes
            gone.update(p for p, i in self.id_map.items() if i in hit and p < n)
        removed = sorted(gone)
        n_new = n - len(removed)
        targets = [p for p in removed if p < n_new]
        movers = [p for p in range(n_new, n) if p not in gone]   # len(removed) candidates at most
        dev = self._dev()
        pos = torch.tensor(removed, dtype=torch.int64, device=dev)
        with self._searcher_lock():
            self._mutate(pos, torch.full_like(pos, -1),
                         torch.zeros((len(removed), self.dimension), dtype=self.storage_dtype, device=dev), n)
            if movers:
                src = torch.tensor(movers, dtype=torch.int64, device=dev)
                dst = torch.tensor(targets, dtype=torch.int64, device=dev)
                slots = self.pos_slot[src]
                self.row_pos[slots.long()] = dst.to(torch.int32)
                self.pos_slot[dst] = slots
                self.assign[dst] = self.assign[src]
                self.pos_slot[src] = -1
                self.assign[src] = -1
                if self._tags is not None:   # the tags follow their items to the positions they fill
                    self._tags[dst] = self._tags[src]
            for p in removed:
                item_id = self.id_map.pop(p, None)
                if item_id is not None and self.reverse_id_map.get(item_id) == p:
                    del self.reverse_id_map[item_id]
            for p, t in zip(movers, targets):
                item_id = self.id_map.pop(p, None)
                if item_id is not None:
                    self.id_map[t] = item_id
                    if self.reverse_id_map.get(item_id) == p:
                        self.reverse_id_map[item_id] = t
                self._ids[t] = self._ids[p]
            del self._ids[n_new:]
            self.current_size = n_new
            self._generation += 1   # positions moved: resident searchers and seen lists remap
        logger.info("Removed %d items from index. Total size: %d", len(removed), n_new)
        return len(removed)

    def vectors(self) -> np.ndarray:
        """The live rows in position order (fp32)."""
        if self._flat is not None:
            return self._flat.vectors()
        if self.index is None or self.current_size == 0:
            return np.zeros((0, self.dimension), np.float32)
        return kernels.gather_rows(self.index, self.pos_slot[: self.current_size].long()).float().cpu().numpy()


# Backwards-compatible name: configs with index_type "faiss" get the exact
# HBM-resident index (Faiss-CPU is not part of the MI355X build).
FaissIndex = HipFlatIPIndex

_INDEX_TYPES = {"hip_flat": HipFlatIPIndex, "faiss": HipFlatIPIndex, "hip_flat_sharded": HipShardedFlatIPIndex,
                "hip_ivf": HipIVFFlatIndex, "hip_ivf_mutable": HipMutableIVFFlatIndex}


def register_index(name: str, cls):
    """Plugin hook: make ``RetrievalEngine(config)`` accept ``index_type=name``."""
    _INDEX_TYPES[name] = cls


class RetrievalEngine:
    """High-level retrieval engine with md5 query cache and metrics
    (retrieval.py:505-692)."""

    def __init__(self, config: Dict[str, Any]):
        self.config = config
        self.index_type = config.get("index_type", "faiss")
        self.top_k = config.get("top_k", 100)
        self.update_interval = config.get("update_interval_seconds", 300)
        self.index = self._create_index()
        self.cache: Dict[str, Dict[str, Any]] = {}
        self.cache_ttl = config.get("cache_ttl", 300)
        self.last_cache_clear = time.time()
        self.total_queries = 0
        self.cache_hits = 0
        self.total_latency = 0.0

    def _create_index(self) -> IndexBase:
        """retrieval.py:532-544 string dispatch (+ the "hip_flat" type)."""
        index_config = dict(self.config.get(self.index_type, {}) or {})
        index_config["dimension"] = self.config.get("embedding_dim", 128)
        cls = _INDEX_TYPES.get(self.index_type)
        if cls is None:
            raise ValueError(f"Unknown index type: {self.index_type}")
        return cls(index_config)

    def build_index(self, embeddings: Array, ids: List[str], item_categories=None):
        """``item_categories``: as ``HipFlatIPIndex.build`` (config key ``categories`` of the index)."""
        if item_categories is None:
            self.index.build(embeddings, ids)
        else:
            self.index.build(embeddings, ids, item_categories=item_categories)
        self.cache.clear()
        logger.info("Built index with %d items", len(embeddings))

    def retrieve(self, query_embeddings: Array, k: Optional[int] = None,
                 filter_ids: Optional[List[str]] = None, use_cache: bool = True, exclude_ids=None,
                 filter_categories=None, exclude_categories=None,
                 mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None
                 ) -> Tuple[List[List[str]], List[List[float]], Dict[str, Any]]:
        """``exclude_ids``: as ``HipFlatIPIndex.search``; like ``filter_ids`` it keeps
        the call out of the query cache (neither read nor filled), and so do
        ``filter_categories`` / ``exclude_categories`` (as ``HipFlatIPIndex.search``)
        and ``mmr_lambda`` / ``mmr_candidates`` — the ranking stage of the request
        path (src/serving/service.py:204-228) as an MMR re-rank of the top
        ``mmr_candidates`` (default ``min(10 * k, 128, index size)``) into k, as
        ``HipFlatIPIndex.search`` describes it."""
        start = time.time()
        k = k or self.top_k
        cache_key = None
        cats = {key: v for key, v in (("filter_categories", filter_categories),
                                      ("exclude_categories", exclude_categories),
                                      ("mmr_lambda", mmr_lambda), ("mmr_candidates", mmr_candidates))
                if v is not None}
        if use_cache and filter_ids is None and exclude_ids is None and not cats:
            qb = query_embeddings.detach().cpu().numpy().tobytes() if isinstance(query_embeddings, torch.Tensor) \
                else np.asarray(query_embeddings).tobytes()
            cache_key = hashlib.md5(qb).hexdigest()
            entry = self.cache.get(cache_key)
            if entry is not None and time.time() - entry["timestamp"] < self.cache_ttl:
                self.cache_hits += 1
                latency = time.time() - start
                self.total_queries += 1
                self.total_latency += latency
                return entry["ids"], entry["scores"], {"latency_ms": latency * 1000, "cache_hit": True}
        if exclude_ids is None:
            item_ids, scores = self.index.search(query_embeddings, k, filter_ids, **cats)
        else:  # HipFlatIPIndex (the sharded index does not take exclusions)
            item_ids, scores = self.index.search(query_embeddings, k, filter_ids, exclude_ids=exclude_ids, **cats)
        if use_cache and cache_key:
            self.cache[cache_key] = {"ids": item_ids, "scores": scores, "timestamp": time.time()}
            if time.time() - self.last_cache_clear > self.cache_ttl:
                self._clear_expired_cache()
        latency = time.time() - start
        self.total_queries += 1
        self.total_latency += latency
        flat = [s for sl in scores for s in sl]
        metrics = {"latency_ms": latency * 1000, "cache_hit": False,
                   "num_results": sum(len(x) for x in item_ids),
                   "avg_score": float(np.mean(flat)) if flat else float("nan")}
        return item_ids, scores, metrics

    def update_index(self, new_embeddings: Array, new_ids: List[str], upsert: bool = False):
        """retrieval.py:629-641 appends (``index.add``): an item whose embedding
        changed is then stored twice. ``upsert=True`` calls ``index.update``
        instead (a ``mutable`` index overwrites known ids in place and appends
        the rest)."""
        if upsert:
            self.index.update(new_embeddings, new_ids)
        else:
            self.index.add(new_embeddings, new_ids)
        self.cache.clear()

    def remove_items(self, ids: List[str]) -> Optional[int]:
        """Withdraw items (``index.remove``; a ``mutable`` index returns the number
        of rows removed)."""
        removed = self.index.remove(ids)
        self.cache.clear()
        return removed

    def _clear_expired_cache(self):
        now = time.time()
        for key in [k for k, e in self.cache.items() if now - e["timestamp"] > self.cache_ttl]:
            del self.cache[key]
        self.last_cache_clear = now

    def get_metrics(self) -> Dict[str, Any]:
        return {
            "total_queries": self.total_queries,
            "avg_latency_ms": self.total_latency / max(self.total_queries, 1) * 1000,
            "cache_hit_rate": self.cache_hits / max(self.total_queries, 1),
            "cache_size": len(self.cache),
            "index_size": self.index.current_size,
            "index_type": self.index_type,
        }

    def save(self, path: str):
        self.index.save(path)

    def load(self, path: str):
        self.index.load(path)
        self.cache.clear()
