"""Torch-facing wrappers of the HIP C ABI (include/rtrec_hip.h).

Every function here launches hand-written gfx950 kernels from
librtrec_hip.so on torch's current stream; none has a CPU path (CPU tensors
raise). Shapes/dtypes are validated on the host before any launch so a bad
call never reaches the GPU.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import native
from .native import call, ptr, stream_of
from .profiling import TIMER

# ---------------------------------------------------------------------------
# workspace cache (grow-only, per device): no allocation inside hot calls
# ---------------------------------------------------------------------------
_WS = {}


def workspace(device: torch.device, nbytes: int, tag: str = "ws") -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# ---------------------------------------------------------------------------
# row gather (src/training/datasets/movielens.py:108-116; nn.Embedding lookup)
# ---------------------------------------------------------------------------

def gather_rows(table: torch.Tensor, ids: torch.Tensor, row_begin: int = 0,
                out: Optional[torch.Tensor] = None, oob: Optional[torch.Tensor] = None,
                check: bool = False) -> torch.Tensor:
    """``out[r] = table[ids[r] - row_begin]``; ids outside the table give zero rows
    (counted in ``oob`` if given). ``check=True`` raises IndexError on any
    out-of-range id like numpy fancy indexing (costs a device sync)."""
    native.require_device(table, ids, what="gather_rows")
    if ids.dtype != torch.int64:
        ids = ids.to(torch.int64)
    ids = ids.contiguous()
    table = table.contiguous()
    row_shape = table.shape[1:]
    row_bytes = table[0].numel() * table.element_size() if table.shape[0] > 0 else \
        int(torch.tensor(row_shape).prod()) * table.element_size()
    if out is None:
        out = torch.empty((ids.numel(),) + tuple(row_shape), dtype=table.dtype, device=table.device)
    if check and oob is None:
        oob = torch.zeros(1, dtype=torch.int32, device=table.device)
    with TIMER.region("gather_rows", bytes_=2.0 * ids.numel() * row_bytes + 8.0 * ids.numel()):
        call("rt_gather_rows", ptr(table), row_begin, table.shape[0], row_bytes, ptr(ids), ids.numel(),
             ptr(out), ptr(oob), stream_of(table))
    if check and int(oob.item()) != 0:
        raise IndexError(f"{int(oob.item())} ids out of range for table of {table.shape[0]} rows")
    return out.view(tuple(ids.shape) + tuple(row_shape))


def scatter_add_rows(grad_table: torch.Tensor, ids: torch.Tensor, grad_out: torch.Tensor,
                     padding_idx: int = -1) -> torch.Tensor:
    """nn.Embedding backward: grad_table[ids[r]] += grad_out[r] (padding_idx skipped)."""
    native.require_device(grad_table, ids, grad_out, what="scatter_add_rows")
    ids = ids.contiguous().to(torch.int64)
    grad_out = grad_out.contiguous().float()
    call("rt_scatter_add_rows_f32", ptr(grad_table), grad_table.shape[0], grad_table.shape[1], ptr(ids),
         ids.numel(), ptr(grad_out), padding_idx, stream_of(grad_table))
    return grad_table


# ---------------------------------------------------------------------------
# in-place row overwrite / order-preserving removal (the Flat index's update and
# remove, src/serving/retrieval.py:228-246)
# ---------------------------------------------------------------------------

def _row_bytes(t: torch.Tensor, what: str) -> int:
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{what} expects contiguous [rows, width] tensors")
    nbytes = t.shape[1] * t.element_size()
    if nbytes == 0 or nbytes % 16 or t.data_ptr() % 16:
        raise ValueError(f"{what}: rows must be a multiple of 16 bytes and 16-byte aligned "
                         f"(row of {nbytes} bytes at {t.data_ptr():#x})")
    return nbytes


def scatter_rows(src: torch.Tensor, positions: torch.Tensor, dst: torch.Tensor,
                 oob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dst[positions[i]] = src[i]`` (rt_scatter_rows). Positions must be unique;
    one outside ``[0, len(dst))`` is skipped and counted in ``oob`` (int32 [1]) if given."""
    native.require_device(src, positions, dst, oob, what="scatter_rows")
    row_bytes = _row_bytes(src, "scatter_rows")
    if src.dtype != dst.dtype or _row_bytes(dst, "scatter_rows") != row_bytes:
        raise ValueError(f"scatter_rows: src rows {tuple(src.shape)} {src.dtype} do not match dst "
                         f"{tuple(dst.shape)} {dst.dtype}")
    if positions.dtype != torch.int64 or positions.dim() != 1 or positions.numel() != src.shape[0]:
        raise ValueError("scatter_rows: positions must be int64 [len(src)]")
    positions = positions.contiguous()
    call("rt_scatter_rows", ptr(src), src.shape[0], row_bytes, ptr(positions), ptr(dst), dst.shape[0], ptr(oob),
         stream_of(dst))
    return dst


def rows_compact(src: torch.Tensor, keep_bits: torch.Tensor, dst: torch.Tensor,
                 n_kept: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stable compaction of the rows of ``src`` whose bit is set in ``keep_bits``
    (int32/uint32 words, bit j of word w = row 32w + j) into ``dst[:n_kept]``
    (rt_rows_compact; out of place, ``len(dst) >= len(src)``). Returns ``n_kept``,
    a device int64 [1]; nothing is read back to the host."""
    native.require_device(src, keep_bits, dst, n_kept, what="rows_compact")
    row_bytes = _row_bytes(src, "rows_compact")
    if src.dtype != dst.dtype or _row_bytes(dst, "rows_compact") != row_bytes:
        raise ValueError(f"rows_compact: src rows {tuple(src.shape)} {src.dtype} do not match dst "
                         f"{tuple(dst.shape)} {dst.dtype}")
    if keep_bits.dtype not in (torch.int32, torch.uint32) or keep_bits.dim() != 1:
        raise ValueError("rows_compact: keep_bits must be int32/uint32 [words]")
    keep_bits = keep_bits.contiguous()
    if n_kept is None:
        n_kept = torch.empty(1, dtype=torch.int64, device=src.device)
    elif n_kept.dtype != torch.int64 or n_kept.numel() != 1:
        raise ValueError("rows_compact: n_kept must be int64 [1]")
    n = src.shape[0]
    ws = workspace(src.device, native.lib().rt_rows_compact_workspace_bytes(n), "rows_compact")
    with TIMER.region("rows_compact", bytes_=float(2 * n * row_bytes)):
        call("rt_rows_compact", ptr(src), n, row_bytes, ptr(keep_bits), keep_bits.numel(), ptr(dst), dst.shape[0],
             ptr(n_kept), ptr(ws), ws.numel(), stream_of(src))
    return n_kept


# ---------------------------------------------------------------------------
# Faiss normalize_L2 + IndexFlatIP search (src/serving/retrieval.py:86,167,171)
# ---------------------------------------------------------------------------

def l2_renorm_(x: torch.Tensor) -> torch.Tensor:
    """In-place ``faiss.normalize_L2`` on fp32 rows."""
    native.require_device(x, what="l2_renorm_")
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("l2_renorm_ expects a contiguous fp32 [n, d] tensor")
    call("rt_l2_renorm_f32", ptr(x), x.shape[0], x.shape[1], stream_of(x))
    return x


def _exclude_words(exclude_bits: Optional[torch.Tensor], nq: int, contiguous: bool) -> int:
    """Words per row of an exclusion bitmap int32/uint32 ``[nq, words]`` (None: 0);
    ``contiguous``: the caller passes the tensor on as it is."""
    if exclude_bits is None:
        return 0
    ok = exclude_bits.dtype in (torch.int32, torch.uint32) and exclude_bits.shape[0] == nq
    if contiguous and not (ok and exclude_bits.is_contiguous()):
        raise ValueError("exclude_bits must be contiguous int32/uint32 [nq, words]")
    if not ok:
        raise ValueError("exclude_bits must be int32/uint32 [nq, words]")
    return exclude_bits.shape[1]


def _topk_out(out: Optional[Tuple[torch.Tensor, torch.Tensor]], nq: int, k: int, device
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The caller's ``out`` pair, or fresh (scores fp32, ids int64) ``[nq, k]``."""
    if out is not None:
        scores, ids = out
        return scores, ids
    return (torch.empty((nq, k), dtype=torch.float32, device=device),
            torch.empty((nq, k), dtype=torch.int64, device=device))


def flatip_topk(queries: torch.Tensor, items: torch.Tensor, k: int,
                exclude_bits: Optional[torch.Tensor] = None, id_offset: int = 0,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact inner-product top-k: (scores [nq,k] f32, ids [nq,k] int64), ordered by
    (score desc, id asc); unfilled slots are (-FLT_MAX, -1)."""
    native.require_device(queries, items, what="flatip_topk")
    if queries.dim() != 2 or items.dim() != 2 or queries.shape[1] != items.shape[1]:
        raise ValueError(f"shape mismatch: queries {tuple(queries.shape)} items {tuple(items.shape)}")
    if queries.dtype != items.dtype:
        raise TypeError("queries and items must share a dtype")
    if k <= 0:
        raise ValueError("k must be positive")
    if k > TOPK_MAX_K:
        return _flatip_topk_wide(queries, items, k, exclude_bits, id_offset, out)
    queries = queries.contiguous()
    items = items.contiguous()
    nq, d = queries.shape
    nx = items.shape[0]
    dt = native.dtype_code(queries.dtype)
    scores, ids = _topk_out(out, nq, k, queries.device)
    if nq == 0:
        return scores, ids
    if exclude_bits is not None:
        exclude_bits = exclude_bits.contiguous()
    words = _exclude_words(exclude_bits, nq, False)
    nbytes = native.lib().rt_flatip_topk_workspace_bytes(nq, nx, d, dt, k)
    ws = workspace(queries.device, nbytes, "topk")
    with TIMER.region("flatip_topk", flops=2.0 * nq * nx * d,
                      bytes_=float((nq + nx) * d * queries.element_size() + nq * k * 12)):
        call("rt_flatip_topk", ptr(queries), nq, ptr(items) if nx else None, nx, d, dt, k, ptr(exclude_bits),
             words, id_offset, ptr(scores), ptr(ids), ptr(ws), ws.numel(), stream_of(queries))
    return scores, ids


TOPK_MAX_K = 512  # rt_flatip_topk: k <= 512 per launch (include/rtrec_hip.h)

ONLINE_MAX_NQ = 8   # RT_ONLINE_MAX_NQ
ONLINE_MAX_K = 128  # RT_ONLINE_MAX_K


def flatip_topk_online_plan(nq: int, nx: int, d: int, dtype: torch.dtype, k: int) -> Tuple[int, int]:
    """Host-only plan of the online scan (rt_flatip_topk_online_plan):
    ``(blocks, rows_per_block)``; block b owns the contiguous rows
    ``[b * rows_per_block, min(nx, (b + 1) * rows_per_block))``. No device work."""
    out = (ctypes.c_int64 * 2)()
    call("rt_flatip_topk_online_plan", int(nq), int(nx), int(d), native.dtype_code(dtype), int(k),
         ctypes.cast(out, ctypes.c_void_p))
    return int(out[0]), int(out[1])


def flatip_topk_online(queries: torch.Tensor, items: torch.Tensor, k: int,
                       exclude_bits: Optional[torch.Tensor] = None, id_offset: int = 0,
                       out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                       workspace_buf: Optional[torch.Tensor] = None,
                       exclude_lists=None, tag_filter=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`flatip_topk` for 1..8 queries and k <= 128 (rt_flatip_topk_online):
    the same results, from one streaming pass over the corpus — the shape of
    the serving path (one user per request, src/serving/retrieval.py:141-197).
    ``workspace_buf``: a caller-owned uint8 device buffer of at least
    ``rt_flatip_topk_online_workspace_bytes`` (default: the shared grow-only one).

    ``exclude_lists`` (rt_flatip_topk_online_lists; not together with
    ``exclude_bits``): one ``(offsets, items[, rows])`` tuple of device tensors,
    or a sequence of one or two of them — CSR sources the scan reads itself.
    ``offsets`` int64 ``[n_rows + 1]``, ``items`` int32 corpus positions
    ascending within a row (duplicates allowed, positions >= nx ignored),
    ``rows`` optional int64 ``[nq]``: query q skips CSR row ``rows[q]`` (default
    q; a row outside the CSR: nothing) of every source.

    ``tag_filter`` (rt_flatip_topk_online_tags; composes with ``exclude_lists``,
    not with ``exclude_bits``): ``(item_tags, any_of, none_of)`` — 64-bit category
    sets per row ``[nx]`` and per-query masks ``[nq]`` (either may be None: all
    0), int64 or uint64 device tensors. Row p is eligible for query q iff
    ``(any_of[q] == 0 or item_tags[p] & any_of[q]) and not item_tags[p] &
    none_of[q]``; the result is the search over the eligible rows, exact."""
    if exclude_lists is not None and exclude_bits is not None:
        raise ValueError("exclude_bits and exclude_lists are mutually exclusive")
    if tag_filter is not None and exclude_bits is not None:
        raise ValueError("exclude_bits and tag_filter are mutually exclusive (tag_filter_bitmap composes them)")
    sources = _exclusion_sources(exclude_lists, queries)
    tags = _tag_filter(tag_filter, queries, items.shape[0] if items.dim() == 2 else 0, "flatip_topk_online")
    native.require_device(queries, items, what="flatip_topk_online")
    if queries.dim() != 2 or items.dim() != 2 or queries.shape[1] != items.shape[1]:
        raise ValueError(f"shape mismatch: queries {tuple(queries.shape)} items {tuple(items.shape)}")
    if queries.dtype != items.dtype:
        raise TypeError("queries and items must share a dtype")
    if k <= 0:
        raise ValueError("k must be positive")
    if not queries.is_contiguous() or not items.is_contiguous():
        raise ValueError("flatip_topk_online expects contiguous queries and items")
    nq, d = queries.shape
    nx = items.shape[0]
    dt = native.dtype_code(queries.dtype)
    scores, ids = _topk_out(out, nq, k, queries.device)
    if nq == 0:
        return scores, ids
    words = _exclude_words(exclude_bits, nq, True)
    ws = workspace_buf
    if ws is None:
        ws = workspace(queries.device, native.lib().rt_flatip_topk_online_workspace_bytes(nq, nx, d, dt, k),
                       "topk_online")
    if exclude_lists is not None or tags is not None:
        for src in sources:
            native.require_device(*src, what="flatip_topk_online")
        # a source without items excludes nothing (and has no items pointer to give)
        sources = [src for src in sources if src[1].numel()]
        arr = (native.ExclusionLists * native.ONLINE_MAX_EXCL_SOURCES)()
        for a, (offsets, its, rows) in zip(arr, sources):
            a.offsets, a.items, a.n_rows, a.rows = ptr(offsets), ptr(its), offsets.numel() - 1, ptr(rows)
        if tags is not None:
            call("rt_flatip_topk_online_tags", ptr(queries), nq, ptr(items) if nx else None, nx, d, dt, k, arr,
                 len(sources), ctypes.byref(tags), id_offset, ptr(scores), ptr(ids), ptr(ws), ws.numel(),
                 stream_of(queries))
            return scores, ids
        call("rt_flatip_topk_online_lists", ptr(queries), nq, ptr(items) if nx else None, nx, d, dt, k, arr,
             len(sources), id_offset, ptr(scores), ptr(ids), ptr(ws), ws.numel(), stream_of(queries))
        return scores, ids
    call("rt_flatip_topk_online", ptr(queries), nq, ptr(items) if nx else None, nx, d, dt, k, ptr(exclude_bits),
         words, id_offset, ptr(scores), ptr(ids), ptr(ws), ws.numel(), stream_of(queries))
    return scores, ids


def _exclusion_sources(exclude_lists, queries: torch.Tensor):
    """``exclude_lists`` of :func:`flatip_topk_online` as a list of
    ``(offsets, items, rows-or-None)``; ``ValueError`` / ``TypeError`` for a
    malformed one (checked on the host, before any device is needed)."""
    if exclude_lists is None:
        return []
    if len(exclude_lists) and isinstance(exclude_lists[0], torch.Tensor):
        exclude_lists = [exclude_lists]   # one bare (offsets, items[, rows]) tuple
    if not 1 <= len(exclude_lists) <= native.ONLINE_MAX_EXCL_SOURCES:
        raise ValueError(f"exclude_lists: {len(exclude_lists)} sources; one or "
                         f"{native.ONLINE_MAX_EXCL_SOURCES} (offsets, items[, rows]) tuples")
    out = []
    for src in exclude_lists:
        if not 2 <= len(src) <= 3:
            raise ValueError("an exclusion source is (offsets, items) or (offsets, items, rows)")
        offsets, its = src[0], src[1]
        rows = src[2] if len(src) == 3 else None
        if offsets.dtype != torch.int64 or its.dtype != torch.int32:
            raise TypeError("an exclusion source is a CSR of int64 offsets and int32 ascending items")
        if offsets.dim() != 1 or offsets.numel() < 1 or its.dim() != 1 or not offsets.is_contiguous() \
                or not its.is_contiguous():
            raise ValueError("an exclusion source needs contiguous 1-d offsets [n_rows + 1] and items")
        if rows is not None:
            if rows.dtype != torch.int64:
                raise TypeError("exclusion rows must be int64")
            if rows.dim() != 1 or rows.numel() < queries.shape[0] or not rows.is_contiguous():
                raise ValueError(f"exclusion rows must be a contiguous [nq = {queries.shape[0]}] tensor")
        out.append((offsets, its, rows))
    return out


def _tag_filter(tag_filter, queries: torch.Tensor, n_pos: int, what: str):
    """``tag_filter`` of :func:`flatip_topk_online` / :func:`ivf_topk` as a
    ``native.TagFilter`` (None: no filter); ``ValueError`` / ``TypeError`` for a
    malformed one. The struct holds raw pointers: the caller's tuple keeps the
    tensors alive for the call."""
    if tag_filter is None:
        return None
    if len(tag_filter) != 3:
        raise ValueError("tag_filter is (item_tags, any_of, none_of)")
    item_tags, any_of, none_of = tag_filter
    if item_tags is None:
        raise ValueError("tag_filter needs item_tags")
    nq = queries.shape[0]
    for name, t, n in (("item_tags", item_tags, n_pos), ("any_of", any_of, nq), ("none_of", none_of, nq)):
        if t is None:
            continue
        if t.dtype not in (torch.int64, torch.uint64):
            raise TypeError(f"tag_filter: {name} must be int64 or uint64 (64-bit category sets)")
        if t.dim() != 1 or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"tag_filter: {name} must be a contiguous 1-d tensor of at least {n} words")
    native.require_device(item_tags, any_of, none_of, what=what)
    out = native.TagFilter()
    out.item_tags, out.any_of, out.none_of = ptr(item_tags), ptr(any_of), ptr(none_of)
    return out


def tag_filter_bitmap(item_tags: torch.Tensor, any_of: Optional[torch.Tensor], none_of: Optional[torch.Tensor],
                      nq: int, n_items: Optional[int] = None, out: Optional[torch.Tensor] = None,
                      accumulate: bool = False) -> torch.Tensor:
    """The tag filter as an exclusion bitmap (rt_tag_filter_bitmap): int32 ``[nq,
    ceil(n_items / 32)]``, bit p of row q set for every item p < ``n_items`` that
    is NOT eligible for query q — what ``exclude_bits`` of :func:`flatip_topk`,
    :func:`ivf_topk` and :func:`ivf_topk_batch` takes. ``out`` with ``accumulate``:
    OR into an existing bitmap (e.g. one of excluded ids); otherwise every word
    is overwritten, pad bits zero. One thread per word, no ``[nq, n_items]``
    intermediate."""
    n_items = item_tags.numel() if n_items is None else int(n_items)
    nq = int(nq)
    for name, t, n in (("item_tags", item_tags, n_items), ("any_of", any_of, nq), ("none_of", none_of, nq)):
        if t is None:
            continue
        if t.dtype not in (torch.int64, torch.uint64):
            raise TypeError(f"tag_filter_bitmap: {name} must be int64 or uint64 (64-bit category sets)")
        if t.dim() != 1 or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"tag_filter_bitmap: {name} must be a contiguous 1-d tensor of at least {n} words")
    native.require_device(item_tags, any_of, none_of, out, what="tag_filter_bitmap")
    words = (n_items + 31) // 32
    if out is None:
        if accumulate:
            raise ValueError("tag_filter_bitmap: accumulate needs the bitmap to OR into (out)")
        out = torch.empty((nq, words), dtype=torch.int32, device=item_tags.device)
    elif out.dtype not in (torch.int32, torch.uint32) or out.dim() != 2 or out.shape[0] != nq \
            or out.shape[1] < words or not out.is_contiguous():
        raise ValueError(f"out must be contiguous int32/uint32 [{nq}, >= {words}]")
    call("rt_tag_filter_bitmap", ptr(item_tags) if n_items else None, n_items, ptr(any_of), ptr(none_of), nq,
         ptr(out), out.shape[1], 1 if accumulate else 0, stream_of(item_tags))
    return out


def tower_infer(args: "native.TowerInferArgs", stream) -> None:
    """The whole eval-mode tower for 1..8 rows in one launch (rt_tower_infer_f32;
    UserTower.forward as src/serving/service.py:286-293 calls it). ``args`` holds
    raw device pointers: the caller keeps their tensors alive and on a device."""
    call("rt_tower_infer_f32", ctypes.byref(args), stream)


def _flatip_topk_wide(queries, items, k, exclude_bits, id_offset, out):
    """k > 512 (faiss.IndexFlatIP.search takes any k, src/serving/retrieval.py:
    170-171): ceil(k/512) exact passes of rt_flatip_topk, each excluding every
    row the earlier passes returned (rt_exclusion_bitmap over their sorted ids,
    OR-ed with the caller's bitmap). Each pass returns the best remaining rows
    in (score desc, id asc) order, so the concatenation is the exact top-k in
    that order; slots past the corpus are (-FLT_MAX, -1)."""
    nq, nx = queries.shape[0], items.shape[0]
    dev = queries.device
    words = (nx + 31) // 32
    if exclude_bits is not None:
        exclude_bits = exclude_bits.contiguous()
        if _exclude_words(exclude_bits, nq, False) < words:
            raise ValueError("exclude_bits has fewer words than ceil(n_items / 32)")
    parts_s, parts_i = [], []
    found = None  # [nq, m] local row ids returned so far (-1 = none)
    left = k
    bits = exclude_bits
    while left > 0:
        kk = min(TOPK_MAX_K, left)
        ps, pi = flatip_topk(queries, items, kk, exclude_bits=bits, id_offset=id_offset)
        parts_s.append(ps)
        parts_i.append(pi)
        left -= kk
        if left <= 0:
            break
        loc = torch.where(pi >= 0, pi - id_offset, torch.full_like(pi, -1))
        found = loc if found is None else torch.cat([found, loc], dim=1)
        srt = found.sort(dim=1).values.to(torch.int32).contiguous()
        offs = torch.arange(nq + 1, dtype=torch.int64, device=dev) * srt.shape[1]
        new = exclusion_bitmap_csr(offs, srt.reshape(-1), nx)
        bits = new if exclude_bits is None else torch.bitwise_or(new, exclude_bits[:, :words].to(new.dtype))
    scores, ids = torch.cat(parts_s, dim=1), torch.cat(parts_i, dim=1)
    if out is not None:
        out[0].copy_(scores)
        out[1].copy_(ids)
        return out
    return scores, ids


# ---- corpus-sharded search with one corpus-wide threshold per query -------
def shard_sample_stride(n_total: int, nt: int = 128, max_stride: int = 64) -> int:
    """Sampling stride (in 128-row stages) for a corpus of ``n_total`` rows
    spread over shards: the planner's 64 when the corpus holds >= 32 x 64
    stages, else fewer, so that >= 32 stages are sampled in all."""
    stages = max(1, -(-int(n_total) // nt))
    return int(max(1, min(max_stride, stages // 32)))


def flatip_topk_shard_plan(nq: int, n_rows: int, d: int, dtype: torch.dtype, k: int, stride: int):
    """Host-only plan of a shard of ``n_rows`` rows (rt_flatip_topk_shard_plan):
    the (sampled, total) 128-row stage counts rt_flatip_topk_shard_sample would
    report, or None when the shape has no v4 plan. No device work, no sync."""
    counts = (ctypes.c_int64 * 2)()
    rc = native.lib().rt_flatip_topk_shard_plan(int(nq), int(n_rows), int(d), native.dtype_code(dtype), int(k),
                                                int(stride), ctypes.cast(counts, ctypes.c_void_p))
    if rc != 0:
        return None
    return int(counts[0]), int(counts[1])


def flatip_topk_shard_sample(queries: torch.Tensor, items: torch.Tensor, k: int, stride: int):
    """This shard's sample (rt_flatip_topk_shard_sample): per query the union
    of each lane half's 16 largest sampled group maxima [nq, 32] f32
    (descending; a subset of the 32 largest, so thresholds drawn from it are
    at or below the exact ones) and the (sampled, total) 128-row stage counts
    of the shard. None when the shape has no v4 plan (f16/bf16, d <= 128,
    k <= 128, >= 65,536 rows or forced)."""
    native.require_device(queries, items, what="flatip_topk_shard_sample")
    queries, items = queries.contiguous(), items.contiguous()
    nq, d = queries.shape
    dt = native.dtype_code(queries.dtype)
    lib = native.lib()
    nbytes = lib.rt_flatip_topk_shard_workspace_bytes(nq, items.shape[0], d, dt, k)
    if nbytes == 0:
        return None
    ws = workspace(queries.device, nbytes, "topk_shard")
    top = torch.empty((nq, 32), dtype=torch.float32, device=queries.device)
    counts = (ctypes.c_int64 * 2)()
    call("rt_flatip_topk_shard_sample", ptr(queries), nq, ptr(items), items.shape[0], d, dt, k, int(stride), ptr(top),
         ctypes.cast(counts, ctypes.c_void_p), ptr(ws), ws.numel(), stream_of(queries))
    return top, (int(counts[0]), int(counts[1]))


def topk_sample_rank(k: int, sampled: int, stages: int) -> int:
    """Failure-safe rank of a corpus-wide sample (rt_topk_sample_rank): P(the
    rank-th largest sampled group maximum exceeds the k-th score) < 1e-6;
    0 when no rank <= 32 is safe (search from -inf)."""
    r = ctypes.c_int(0)
    call("rt_topk_sample_rank", int(k), int(sampled), int(stages), ctypes.byref(r))
    return int(r.value)


def topk_sample_threshold(lists: torch.Tensor, rank: int) -> torch.Tensor:
    """thr [nq] = the rank-th largest of the union of lists [n_lists, nq, 32]
    (rt_topk_sample_threshold); -FLT_MAX when fewer finite entries."""
    native.require_device(lists, what="topk_sample_threshold")
    lists = lists.contiguous()
    n_lists, nq = lists.shape[0], lists.shape[1]
    thr = torch.empty(nq, dtype=torch.float32, device=lists.device)
    call("rt_topk_sample_threshold", ptr(lists), n_lists, nq, int(rank), ptr(thr), stream_of(lists))
    return thr


def flatip_topk_shard_search(queries: torch.Tensor, items: torch.Tensor, k: int, thr: torch.Tensor,
                             id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """This shard's rows scoring >= thr[q], the best k per query in (score desc,
    id asc) order, (-FLT_MAX, -1) padded (rt_flatip_topk_shard_search)."""
    native.require_device(queries, items, thr, what="flatip_topk_shard_search")
    queries, items, thr = queries.contiguous(), items.contiguous(), thr.contiguous().float()
    nq, d = queries.shape
    dt = native.dtype_code(queries.dtype)
    nbytes = native.lib().rt_flatip_topk_shard_workspace_bytes(nq, items.shape[0], d, dt, k)
    if nbytes == 0:
        raise native.RTError("rt_flatip_topk_shard_search", -2, "no v4 plan for this shape")
    ws = workspace(queries.device, nbytes, "topk_shard")
    scores, ids = _topk_out(None, nq, k, queries.device)
    with TIMER.region("flatip_topk", flops=2.0 * nq * items.shape[0] * d,
                      bytes_=float((nq + items.shape[0]) * d * queries.element_size() + nq * k * 12)):
        call("rt_flatip_topk_shard_search", ptr(queries), nq, ptr(items), items.shape[0], d, dt, k, ptr(thr),
             int(id_offset), ptr(scores), ptr(ids), ptr(ws), ws.numel(), stream_of(queries))
    return scores, ids


def topk_tuning(v4_mode: int = 0, v4_stride: int = 0, v4_rank: int = -1) -> None:
    """Planner override of flatip_topk (rt_flatip_topk_tuning; process-wide,
    results unchanged): v4_mode 0 automatic / 1 never / 2 wherever legal the
    sampled-threshold kernel pair (+4: per-split thresholds instead of one
    corpus-wide threshold per query; +8: small fp32 corpora keep the fused
    register-list scan instead of the score-slab GEMM + select); v4_stride the sample stride in 128-row stages
    (0 = planner); v4_rank the sampled rank (-1 = planner, 0 = no sample)."""
    call("rt_flatip_topk_tuning", int(v4_mode), int(v4_stride), int(v4_rank))


def l2_augment(x: torch.Tensor, role: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, d] fp32 → [n, d+4] augmented rows for the L2 mode (rt_l2_augment_f32):
    role 0 (queries) appends 1, role 1 (items) appends -||x||^2/2."""
    native.require_device(x, what="l2_augment")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("l2_augment expects fp32 [n, d]")
    x = x.contiguous()
    n, d = x.shape
    if out is None:
        out = torch.empty((n, d + 4), dtype=torch.float32, device=x.device)
    call("rt_l2_augment_f32", ptr(x), n, d, ptr(out), out.shape[1], role, stream_of(x))
    return out


def flatl2_topk(q_aug: torch.Tensor, x_aug: torch.Tensor, d: int, k: int,
                exclude_bits: Optional[torch.Tensor] = None, id_offset: int = 0, verify: bool = True
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact squared-L2 k-NN on augmented rows (IndexFlatL2.search): (distances
    [nq, k] ascending, ids [nq, k]); unfilled slots (FLT_MAX, -1). k + 32
    candidates are selected on the augmented inner product and re-ranked on
    Faiss's distance (rt_l2_finish_f32), which certifies every query: a query
    whose k-th distance is within a rounding bound of what an unselected item
    could reach (near-duplicate or clustered corpora) is re-selected with 512
    candidates. ``verify`` costs one device→host read (the flagged count);
    ``L2_STATS`` counts re-selected queries and any left uncertified (only
    possible when more than 512 - k items tie within rounding of the k-th)."""
    nq, nx = q_aug.shape[0], x_aug.shape[0]
    k_sel = min(k + L2_MARGIN, 512)
    s, i = _topk_out(None, nq, k, q_aug.device)
    if nq == 0:
        return s, i
    verify = verify and k_sel < nx  # a selection of the whole corpus is exact by construction
    flags = torch.empty(nq, dtype=torch.int32, device=q_aug.device) if verify else None

    def select_finish(q, bits, ksel, out_s, out_i, out_f):
        sel_s, sel = flatip_topk(q, x_aug, ksel, exclude_bits=bits, id_offset=id_offset)
        call("rt_l2_finish_f32", ptr(q), q.shape[1], ptr(x_aug), x_aug.shape[1], d, q.shape[0], ksel,
             ptr(sel), ptr(sel_s) if out_f is not None else None, k, ptr(out_s), ptr(out_i), ptr(out_f),
             id_offset, stream_of(q))

    select_finish(q_aug, exclude_bits, k_sel, s, i, flags)
    if verify:
        bad = torch.nonzero(flags).flatten()
        nb = bad.numel()
        left = 0
        if nb and k_sel < min(512, nx):
            qb = q_aug.index_select(0, bad).contiguous()
            bb = exclude_bits.index_select(0, bad).contiguous() if exclude_bits is not None else None
            s2, i2 = _topk_out(None, nb, k, q_aug.device)
            k2 = min(512, nx)
            # a re-selection of the whole corpus is exact by construction: no certificate
            f2 = torch.empty(nb, dtype=torch.int32, device=q_aug.device) if k2 < nx else None
            select_finish(qb, bb, k2, s2, i2, f2)
            s.index_copy_(0, bad, s2)
            i.index_copy_(0, bad, i2)
            left = int(f2.sum().item()) if f2 is not None else 0
        elif nb:
            left = nb
        L2_STATS["reselected"] += nb if k_sel < min(512, nx) else 0
        L2_STATS["uncertified"] += left
    return s, i


L2_MARGIN = 32  # over-selected candidates per query in the L2 mode
L2_STATS = {"reselected": 0, "uncertified": 0}  # flatl2_topk certificate outcomes (process-wide)


def topk_merge(scores: torch.Tensor, ids: torch.Tensor, k_out: int
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge candidate lists [n_lists, nq, k_in] into the (score desc, id asc) top k_out."""
    native.require_device(scores, ids, what="topk_merge")
    scores = scores.contiguous().float()
    ids = ids.contiguous().to(torch.int64)
    n_lists, nq, k_in = scores.shape
    os_, oi = _topk_out(None, nq, k_out, scores.device)
    call("rt_topk_merge", ptr(scores), ptr(ids), nq, n_lists, k_in, k_out, ptr(os_), ptr(oi),
         stream_of(scores))
    return os_, oi


MMR_MAX_CAND = 128   # RT_MMR_MAX_CAND


def mmr_rerank(scores: torch.Tensor, positions: torch.Tensor, rows: torch.Tensor, k: int, lam,
               pos_slot: Optional[torch.Tensor] = None, n_pos: Optional[int] = None, normalize: bool = False,
               out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Maximal Marginal Relevance over retrieved candidates (rt_mmr_rerank): per
    query a greedy choice of ``k`` of the ``n_cand <= 128`` candidates
    ``(scores, positions)`` ``[nq, n_cand]`` a search returned, maximising
    ``lam * score - (1 - lam) * max similarity to what is already chosen``; ties go
    to the lower candidate index. Returns the chosen candidates' original
    (scores, positions) ``[nq, k]`` in selection order, ``(-FLT_MAX, -1)`` past the
    number of present candidates.

    ``rows`` ``[n_rows, d]``: the stored embeddings (fp32 / fp16 / bf16).
    ``pos_slot``: optional int32 ``[n_pos]``, the stored row of a position (-1:
    none); None: the identity. ``n_pos``: positions are valid in ``[0, n_pos)``
    (default: ``len(pos_slot)``, else ``len(rows)``). ``lam``: a float, or an fp32
    device tensor ``[nq]`` (one value per query; read by the kernel, so a captured
    call follows a value changed in place). ``normalize``: similarities are
    cosines of the stored rows instead of their inner products."""
    native.require_device(scores, positions, rows, pos_slot, lam if isinstance(lam, torch.Tensor) else None,
                          what="mmr_rerank")
    if scores.dim() != 2 or positions.shape != scores.shape or rows.dim() != 2:
        raise ValueError(f"shape mismatch: scores {tuple(scores.shape)} positions {tuple(positions.shape)} "
                         f"rows {tuple(rows.shape)}")
    if scores.dtype != torch.float32 or positions.dtype != torch.int64:
        raise TypeError("mmr_rerank expects fp32 scores and int64 positions")
    if not (scores.is_contiguous() and positions.is_contiguous() and rows.is_contiguous()):
        raise ValueError("mmr_rerank expects contiguous scores, positions and rows")
    nq, n_cand = scores.shape
    if not 0 < k <= n_cand:
        raise ValueError(f"mmr_rerank: need 0 < k <= n_cand, got k={k}, n_cand={n_cand}")
    if n_cand > MMR_MAX_CAND:
        raise ValueError(f"mmr_rerank: at most {MMR_MAX_CAND} candidates per query, got {n_cand}")
    if pos_slot is not None and (pos_slot.dtype != torch.int32 or pos_slot.dim() != 1
                                 or not pos_slot.is_contiguous()):
        raise TypeError("mmr_rerank: pos_slot must be a contiguous int32 vector")
    if n_pos is None:
        n_pos = pos_slot.numel() if pos_slot is not None else rows.shape[0]
    if n_pos < 0 or (pos_slot is not None and n_pos > pos_slot.numel()):
        raise ValueError("mmr_rerank: n_pos outside pos_slot")
    if isinstance(lam, torch.Tensor):
        if lam.dtype != torch.float32 or lam.dim() != 1 or lam.numel() < nq or not lam.is_contiguous():
            raise ValueError("mmr_rerank: lam must be a float or a contiguous fp32 tensor [nq]")
    else:
        lam = torch.full((max(nq, 1),), float(lam), dtype=torch.float32, device=scores.device)
    os_, oi = _topk_out(out, nq, k, scores.device)
    if nq == 0:
        return os_, oi
    n_rows, d = rows.shape
    call("rt_mmr_rerank", ptr(scores), ptr(positions), nq, n_cand, ptr(rows) if n_rows else None, n_rows, d,
         native.dtype_code(rows.dtype), ptr(pos_slot), int(n_pos), ptr(lam), int(bool(normalize)), int(k),
         ptr(os_), ptr(oi), stream_of(scores))
    return os_, oi


# ---------------------------------------------------------------------------
# IVF-Flat (faiss "IVF<nlist>,Flat" + nprobe, src/serving/retrieval.py:60-62,101-133)
# ---------------------------------------------------------------------------

IVF_MAX_K = 128        # RT_IVF_MAX_K
IVF_MAX_NPROBE = 128   # RT_IVF_MAX_NPROBE
IVF_QUERY_CHUNK = 32768  # queries per rt_ivf_topk call (the kernel's grid takes 65,535)


def ivf_topk_plan(nq: int, nprobe: int, max_list_rows: int) -> Tuple[int, int, int]:
    """Host-only plan of the probed-list scan (rt_ivf_topk_plan): ``(chunks per
    list, rows per chunk, scan blocks)``. No device work."""
    out = (ctypes.c_int64 * 3)()
    call("rt_ivf_topk_plan", int(nq), int(nprobe), int(max_list_rows), ctypes.cast(out, ctypes.c_void_p))
    return int(out[0]), int(out[1]), int(out[2])


def ivf_topk_tuning(min_chunk_tiles: int = 0) -> None:
    """Floor of the scan's chunk in 256-row tiles (0 = default); for measurements."""
    call("rt_ivf_topk_tuning", int(min_chunk_tiles))


def ivf_topk(queries: torch.Tensor, rows: torch.Tensor, list_offsets: torch.Tensor, row_pos: torch.Tensor,
             probes: torch.Tensor, max_list_rows: int, k: int, exclude_bits: Optional[torch.Tensor] = None,
             out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
             workspace_buf: Optional[torch.Tensor] = None,
             exclude_lists=None, list_len: Optional[torch.Tensor] = None,
             n_pos: Optional[int] = None, tag_filter=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k over the union of the probed lists (rt_ivf_topk): (scores [nq, k] f32,
    original positions [nq, k] int64) in (score desc, position asc) order,
    (-FLT_MAX, -1) pads. ``rows`` [nx, d] are stored list-contiguous, list l =
    stored rows ``[list_offsets[l], list_offsets[l + 1])``; ``row_pos`` int32 [nx]
    = original position of each stored row; ``probes`` int64 [nq, nprobe] list
    ids (-1: skipped); ``exclude_bits`` is indexed by original position.
    ``exclude_lists`` (rt_ivf_topk_lists; not together with ``exclude_bits``):
    the forms of :func:`flatip_topk_online`'s — one or two ``(offsets, items[,
    rows])`` CSR sources of ORIGINAL positions that the scan reads itself.
    ``list_len`` (int64 [nlist]) with ``n_pos``: lists stored with slack
    (rt_ivf_topk_lens / rt_ivf_topk_lists_lens) — list l's live rows are the first
    ``list_len[l]`` of its ``[list_offsets[l], list_offsets[l + 1])``, positions
    are valid in ``[0, n_pos)`` (the bitmap's width), ``max_list_rows`` bounds the
    largest capacity.
    ``tag_filter`` (rt_ivf_topk_tags; composes with ``exclude_lists``, not with
    ``exclude_bits``): ``(item_tags, any_of, none_of)`` as for
    :func:`flatip_topk_online`, ``item_tags`` indexed by ORIGINAL position. The
    result is exact over the eligible rows of the PROBED lists (as a filtered
    Faiss IVF search is), not of the corpus.
    Batches above 32,768 queries run in chunks."""
    if exclude_lists is not None and exclude_bits is not None:
        raise ValueError("exclude_bits and exclude_lists are mutually exclusive")
    if tag_filter is not None and exclude_bits is not None:
        raise ValueError("exclude_bits and tag_filter are mutually exclusive (tag_filter_bitmap composes them)")
    sources = _exclusion_sources(exclude_lists, queries)
    tags = _tag_filter(tag_filter, queries,
                       int(n_pos) if n_pos is not None else (rows.shape[0] if rows.dim() == 2 else 0), "ivf_topk")
    native.require_device(queries, rows, list_offsets, row_pos, probes, exclude_bits, list_len, what="ivf_topk")
    for src in sources:
        native.require_device(*src, what="ivf_topk")
    # a source without items excludes nothing (and has no items pointer to give)
    sources = [src for src in sources if src[1].numel()]
    if queries.dim() != 2 or rows.dim() != 2 or queries.shape[1] != rows.shape[1]:
        raise ValueError(f"shape mismatch: queries {tuple(queries.shape)} rows {tuple(rows.shape)}")
    if queries.dtype != rows.dtype:
        raise TypeError("queries and rows must share a dtype")
    if not 1 <= k <= IVF_MAX_K:
        raise ValueError(f"k={k}: ivf_topk returns 1..{IVF_MAX_K} results per query")
    if not (queries.is_contiguous() and rows.is_contiguous() and probes.is_contiguous()
            and list_offsets.is_contiguous() and row_pos.is_contiguous()):
        raise ValueError("ivf_topk expects contiguous operands")
    nq, d = queries.shape
    nx = rows.shape[0]
    if list_offsets.dtype != torch.int64 or list_offsets.dim() != 1 or list_offsets.numel() < 2:
        raise ValueError("list_offsets must be int64 [nlist + 1]")
    if row_pos.dtype != torch.int32 or row_pos.numel() != nx:
        raise ValueError("row_pos must be int32 [nx]")
    if probes.dtype != torch.int64 or probes.dim() != 2 or probes.shape[0] != nq:
        raise ValueError("probes must be int64 [nq, nprobe]")
    nprobe = probes.shape[1]
    if not 1 <= nprobe <= IVF_MAX_NPROBE:
        raise ValueError(f"nprobe={nprobe}: 1..{IVF_MAX_NPROBE}")
    nlist = list_offsets.numel() - 1
    lens = ()   # the two operands the _lens entry points take behind nlist
    if list_len is not None:
        if list_len.dtype != torch.int64 or list_len.numel() != nlist or not list_len.is_contiguous():
            raise ValueError("list_len must be contiguous int64 [nlist]")
        if n_pos is None or not 0 <= int(n_pos):
            raise ValueError("list_len comes with n_pos >= 0, the number of valid positions")
        lens = (ptr(list_len), int(n_pos))
    elif n_pos is not None:
        raise ValueError("n_pos comes with list_len")
    suffix = "_lens" if lens else ""
    dt = native.dtype_code(queries.dtype)
    scores, ids = _topk_out(out, nq, k, queries.device)
    words = _exclude_words(exclude_bits, nq, True)
    for a in range(0, nq, IVF_QUERY_CHUNK):
        b = min(nq, a + IVF_QUERY_CHUNK)
        ws = workspace_buf
        if ws is None:
            ws = workspace(queries.device,
                           native.lib().rt_ivf_topk_workspace_bytes(b - a, nprobe, int(max_list_rows), k), "ivf_topk")
        if exclude_lists is not None or tags is not None:
            # query a + q of the chunk: rows[a + q] of a source with rows, else CSR row a + q —
            # the offsets advanced by a (a source the chunk lies past: dropped)
            arr = (native.ExclusionLists * native.ONLINE_MAX_EXCL_SOURCES)()
            n_src = 0
            for offsets, its, xrows in sources:
                n_rows = offsets.numel() - 1
                if xrows is None:
                    if n_rows - a <= 0:
                        continue
                    offsets, n_rows = offsets[a:], n_rows - a
                else:
                    xrows = xrows[a:b]
                s = arr[n_src]
                s.offsets, s.items, s.n_rows, s.rows = ptr(offsets), ptr(its), n_rows, ptr(xrows)
                n_src += 1
            if tags is not None:
                chunk = native.TagFilter()
                chunk.item_tags = tags.item_tags
                chunk.any_of = ptr(tag_filter[1][a:b]) if tag_filter[1] is not None else None
                chunk.none_of = ptr(tag_filter[2][a:b]) if tag_filter[2] is not None else None
                call("rt_ivf_topk_tags", ptr(queries[a:b]), b - a, ptr(rows) if nx else None, nx, d, dt,
                     ptr(list_offsets), nlist, ptr(list_len), int(n_pos) if lens else nx,
                     ptr(row_pos) if nx else None, ptr(probes[a:b]), nprobe, int(max_list_rows), k, arr, n_src,
                     ctypes.byref(chunk), ptr(scores[a:b]), ptr(ids[a:b]), ptr(ws), ws.numel(), stream_of(queries))
                continue
            call("rt_ivf_topk_lists" + suffix, ptr(queries[a:b]), b - a, ptr(rows) if nx else None, nx, d, dt,
                 ptr(list_offsets), nlist, *lens, ptr(row_pos) if nx else None, ptr(probes[a:b]), nprobe,
                 int(max_list_rows), k, arr, n_src, ptr(scores[a:b]), ptr(ids[a:b]), ptr(ws), ws.numel(),
                 stream_of(queries))
            continue
        call("rt_ivf_topk" + suffix, ptr(queries[a:b]), b - a, ptr(rows) if nx else None, nx, d, dt,
             ptr(list_offsets), nlist, *lens, ptr(row_pos) if nx else None, ptr(probes[a:b]), nprobe,
             int(max_list_rows), k, ptr(exclude_bits[a:b]) if exclude_bits is not None else None, words,
             ptr(scores[a:b]), ptr(ids[a:b]), ptr(ws), ws.numel(), stream_of(queries))
    return scores, ids


# Workspace one rt_ivf_topk_batch call may take; larger batches run in query
# chunks. A policy default (the partial lists of a chunk stay inside the 256 MB
# Infinity Cache), not a measured one.
IVF_BATCH_WORKSPACE_BUDGET = 256 << 20


def ivf_topk_batch_plan(nq: int, nprobe: int, nlist: int, max_list_rows: int, k: int
                        ) -> Tuple[int, int, int, int, int]:
    """Host-only plan of the list-major batch search (rt_ivf_topk_batch_plan):
    ``(QT, rows per chunk, chunks per list, upper bound of the work items, scan
    blocks launched)``. No device work."""
    out = (ctypes.c_int64 * 5)()
    call("rt_ivf_topk_batch_plan", int(nq), int(nprobe), int(nlist), int(max_list_rows), int(k),
         ctypes.cast(out, ctypes.c_void_p))
    return tuple(int(v) for v in out)


def ivf_topk_batch_tuning(stages: int = 0) -> None:
    """Which stages a batch call issues (1 grouping | 2 scan | 4 finish; 0 = all): for
    measuring a stage alone over the workspace of an earlier whole call."""
    call("rt_ivf_topk_batch_tuning", int(stages))


def _ivf_batch_query_chunk(nq: int, nprobe: int, nlist: int, max_list_rows: int, k: int) -> int:
    """Largest number of queries whose workspace fits IVF_BATCH_WORKSPACE_BUDGET
    (at least one tile of 32; the workspace is monotone in nq)."""
    size = native.lib().rt_ivf_topk_batch_workspace_bytes
    if size(nq, nprobe, nlist, max_list_rows, k) <= IVF_BATCH_WORKSPACE_BUDGET:
        return nq
    lo, hi = 1, max(1, nq // 32)   # in tiles: lo always runs, hi does not fit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if size(32 * mid, nprobe, nlist, max_list_rows, k) <= IVF_BATCH_WORKSPACE_BUDGET:
            lo = mid
        else:
            hi = mid
    return min(nq, 32 * lo)


def ivf_topk_batch(queries: torch.Tensor, rows: torch.Tensor, list_offsets: torch.Tensor, row_pos: torch.Tensor,
                   probes: torch.Tensor, max_list_rows: int, k: int, exclude_bits: Optional[torch.Tensor] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   workspace_buf: Optional[torch.Tensor] = None,
                   list_len: Optional[torch.Tensor] = None, n_pos: Optional[int] = None,
                   exclude_lists=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`ivf_topk` for large batches (rt_ivf_topk_batch): the same operands
    and, bit for bit, the same (scores [nq, k] f32, original positions [nq, k]
    int64) — but the work is grouped by LIST: a block scans a chunk of a list
    once for a tile of 32 queries that probe it, on the fp32 MFMA, where
    ``ivf_topk`` streams the list again for every (query, probe) pair.
    ``list_len`` with ``n_pos``: lists stored with slack, as for ``ivf_topk``.
    ``exclude_bits`` is indexed by original position. CSR ``exclude_lists`` are
    not taken: use :func:`ivf_topk`, the small-call path, for those.
    Queries run in chunks whose workspace stays within
    ``IVF_BATCH_WORKSPACE_BUDGET`` (256 MiB by default: a policy default, not a
    measured one); a ``workspace_buf`` must hold one whole call's workspace."""
    if exclude_lists is not None:
        raise ValueError("ivf_topk_batch takes exclude_bits only; CSR exclude_lists are read by ivf_topk")
    native.require_device(queries, rows, list_offsets, row_pos, probes, exclude_bits, list_len, what="ivf_topk_batch")
    if queries.dim() != 2 or rows.dim() != 2 or queries.shape[1] != rows.shape[1]:
        raise ValueError(f"shape mismatch: queries {tuple(queries.shape)} rows {tuple(rows.shape)}")
    if queries.dtype != rows.dtype:
        raise TypeError("queries and rows must share a dtype")
    if not 1 <= k <= IVF_MAX_K:
        raise ValueError(f"k={k}: ivf_topk_batch returns 1..{IVF_MAX_K} results per query")
    if not (queries.is_contiguous() and rows.is_contiguous() and probes.is_contiguous()
            and list_offsets.is_contiguous() and row_pos.is_contiguous()):
        raise ValueError("ivf_topk_batch expects contiguous operands")
    nq, d = queries.shape
    nx = rows.shape[0]
    if list_offsets.dtype != torch.int64 or list_offsets.dim() != 1 or list_offsets.numel() < 2:
        raise ValueError("list_offsets must be int64 [nlist + 1]")
    if row_pos.dtype != torch.int32 or row_pos.numel() != nx:
        raise ValueError("row_pos must be int32 [nx]")
    if probes.dtype != torch.int64 or probes.dim() != 2 or probes.shape[0] != nq:
        raise ValueError("probes must be int64 [nq, nprobe]")
    nprobe = probes.shape[1]
    if not 1 <= nprobe <= IVF_MAX_NPROBE:
        raise ValueError(f"nprobe={nprobe}: 1..{IVF_MAX_NPROBE}")
    nlist = list_offsets.numel() - 1
    if list_len is not None:
        if list_len.dtype != torch.int64 or list_len.numel() != nlist or not list_len.is_contiguous():
            raise ValueError("list_len must be contiguous int64 [nlist]")
        if n_pos is None or not 0 <= int(n_pos):
            raise ValueError("list_len comes with n_pos >= 0, the number of valid positions")
    elif n_pos is not None:
        raise ValueError("n_pos comes with list_len")
    dt = native.dtype_code(queries.dtype)
    scores, ids = _topk_out(out, nq, k, queries.device)
    words = _exclude_words(exclude_bits, nq, True)
    mlr = int(max_list_rows)
    size = native.lib().rt_ivf_topk_batch_workspace_bytes
    if workspace_buf is not None:
        step = nq
    else:
        step = _ivf_batch_query_chunk(nq, nprobe, nlist, mlr, k) if nq else 0
    for a in range(0, nq, max(step, 1)):
        b = min(nq, a + step)
        ws = workspace_buf
        if ws is None:
            ws = workspace(queries.device, size(b - a, nprobe, nlist, mlr, k), "ivf_topk_batch")
        call("rt_ivf_topk_batch", ptr(queries[a:b]), b - a, ptr(rows) if nx else None, nx, d, dt,
             ptr(list_offsets), nlist, ptr(list_len) if list_len is not None else None,
             int(n_pos) if list_len is not None else nx, ptr(row_pos) if nx else None, ptr(probes[a:b]), nprobe,
             mlr, k, ptr(exclude_bits[a:b]) if exclude_bits is not None else None, words,
             ptr(scores[a:b]), ptr(ids[a:b]), ptr(ws), ws.numel(), stream_of(queries))
    return scores, ids


def ivf_lists_update(rows: torch.Tensor, list_offsets: torch.Tensor, list_len: torch.Tensor, row_pos: torch.Tensor,
                     pos_slot: torch.Tensor, assign: torch.Tensor, positions: torch.Tensor, new_list: torch.Tensor,
                     new_rows: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One batch of in-place list mutations (rt_ivf_lists_update) on lists stored
    with slack: operation i overwrites the row of ``positions[i]`` (unique, int64)
    where it lies when its list stays ``new_list[i]``, otherwise moves it to that
    list, ``new_list[i] == -1`` withdrawing it; ``new_rows`` [m, d] in the dtype of
    ``rows``. Stream-ordered, nothing is read back. Returns ``status`` (int32 [2],
    device): all or nothing — ``status[0]`` lists that would overflow their
    capacity, ``status[1]`` refused operations; non-zero means no state changed."""
    native.require_device(rows, list_offsets, list_len, row_pos, pos_slot, assign, positions, new_list, new_rows,
                          status, what="ivf_lists_update")
    _row_bytes(rows, "ivf_lists_update")
    total, d = rows.shape
    m = positions.numel()
    if new_rows.dtype != rows.dtype or new_rows.dim() != 2 or tuple(new_rows.shape) != (m, d) \
            or not new_rows.is_contiguous():
        raise ValueError(f"ivf_lists_update: new_rows must be contiguous {rows.dtype} [{m}, {d}]")
    nlist = list_offsets.numel() - 1
    for t, dt_, n, what in ((list_offsets, torch.int64, nlist + 1, "list_offsets"),
                            (list_len, torch.int64, nlist, "list_len"),
                            (row_pos, torch.int32, total, "row_pos"), (pos_slot, torch.int32, total, "pos_slot"),
                            (assign, torch.int64, total, "assign"), (positions, torch.int64, m, "positions"),
                            (new_list, torch.int64, m, "new_list")):
        if t.dtype != dt_ or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"ivf_lists_update: {what} must be contiguous {dt_} [{n}]")
    if nlist < 1:
        raise ValueError("ivf_lists_update: list_offsets must be int64 [nlist + 1]")
    if status is None:
        status = torch.empty(2, dtype=torch.int32, device=rows.device)
    elif status.dtype != torch.int32 or status.numel() != 2 or not status.is_contiguous():
        raise ValueError("ivf_lists_update: status must be int32 [2]")
    if m == 0:
        return status.zero_()
    ws = workspace(rows.device, native.lib().rt_ivf_lists_update_workspace_bytes(nlist, m), "ivf_lists_update")
    call("rt_ivf_lists_update", ptr(rows), total, d, native.dtype_code(rows.dtype), ptr(list_offsets), nlist,
         ptr(list_len), ptr(row_pos), ptr(pos_slot), ptr(assign), ptr(positions), ptr(new_list), ptr(new_rows), m,
         ptr(status), ptr(ws), ws.numel(), stream_of(rows))
    return status


def segment_mean(rows: torch.Tensor, offsets: torch.Tensor, prev: torch.Tensor, normalize: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n_seg, d] means of the row segments ``[offsets[s], offsets[s + 1])`` of
    ``rows`` [n, d] (rt_segment_mean_f32: fp64 accumulation in a fixed order, no
    atomics); an empty segment copies ``prev[s]``; ``normalize`` rescales the
    non-empty results to unit L2 norm."""
    native.require_device(rows, offsets, prev, out, what="segment_mean")
    if rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("segment_mean expects contiguous [n, d] rows")
    n, d = rows.shape
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1 or not offsets.is_contiguous():
        raise ValueError("offsets must be contiguous int64 [n_seg + 1]")
    n_seg = offsets.numel() - 1
    if prev.dtype != torch.float32 or tuple(prev.shape) != (n_seg, d) or not prev.is_contiguous():
        raise ValueError(f"prev must be contiguous fp32 [{n_seg}, {d}]")
    if out is None:
        out = torch.empty((n_seg, d), dtype=torch.float32, device=rows.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n_seg, d) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 [{n_seg}, {d}]")
    call("rt_segment_mean_f32", ptr(rows) if n else None, n, d, native.dtype_code(rows.dtype), ptr(offsets), n_seg,
         ptr(prev), 1 if normalize else 0, ptr(out), stream_of(rows))
    return out


def exclusion_bitmap(n_queries: int, n_items: int, excluded, device) -> torch.Tensor:
    """int32 bitmap [nq, ceil(n_items/32)] (bit j of row q set ⇒ item j skipped for
    query q) from per-query excluded item lists — the train-item mask of
    scripts/evaluate_model.py:225-228. Host-side construction."""
    import numpy as np
    words = (n_items + 31) // 32
    mask = np.zeros((n_queries, words * 32), dtype=bool)
    for q, items in enumerate(excluded):
        sel = [int(i) for i in items if 0 <= int(i) < n_items]
        if sel:
            mask[q, sel] = True
    packed = np.packbits(mask, axis=1, bitorder="little")  # little-endian words: bit j = item j
    return torch.from_numpy(np.ascontiguousarray(packed).view(np.int32).copy()).to(device)


def exclusion_bitmap_csr(offsets: torch.Tensor, items: torch.Tensor, n_items: int,
                         rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device exclusion bitmap (rt_exclusion_bitmap): row r masks the items of CSR
    row ``rows[r]`` (or r) — the train-item -inf mask of generate_recommendations
    (scripts/evaluate_model.py:224-228). int32 [n_rows, ceil(n_items/32)]."""
    native.require_device(offsets, items, what="exclusion_bitmap_csr")
    if offsets.dtype != torch.int64 or items.dtype != torch.int32:
        raise TypeError("CSR must be int64 offsets and int32 sorted items")
    n_csr = offsets.numel() - 1
    if rows is not None:
        rows = rows.contiguous().to(torch.int64)
    n_rows = rows.numel() if rows is not None else n_csr
    words = (n_items + 31) // 32
    if out is None:
        out = torch.empty((n_rows, words), dtype=torch.int32, device=offsets.device)
    call("rt_exclusion_bitmap", ptr(offsets), ptr(items), n_csr, ptr(rows), n_rows, n_items, ptr(out), words,
         stream_of(offsets))
    return out


def rank_metrics(preds: torch.Tensor, gt_offsets: torch.Tensor, gt_items: torch.Tensor, k_values,
                 gt_rows: Optional[torch.Tensor] = None, ex_offsets: Optional[torch.Tensor] = None,
                 ex_items: Optional[torch.Tensor] = None, ex_rows: Optional[torch.Tensor] = None,
                 num_items: int = 0):
    """Ranking metrics of Evaluator.evaluate (src/evaluation/metrics.py:248-319) on
    the device (rt_rank_metrics + rt_rank_metrics_reduce). Returns (per_row fp64
    [n, 4·n_k+2], valid int32 [n], summary fp64 [4·n_k+4] = column means over
    valid rows, n_valid, coverage)."""
    native.require_device(preds, gt_offsets, gt_items, what="rank_metrics")
    preds = preds.contiguous().to(torch.int64)
    if preds.dim() != 2:
        raise ValueError("preds must be [n_rows, list_len]")
    ks = [int(k) for k in k_values]
    if not ks or len(ks) > native.RT_METRICS_MAX_K or sorted(set(ks)) != ks or ks[0] <= 0:
        raise ValueError(f"k_values must be 1..{native.RT_METRICS_MAX_K} ascending positive ints")
    for t, dt in ((gt_offsets, torch.int64), (gt_items, torch.int32), (ex_offsets, torch.int64),
                  (ex_items, torch.int32)):
        if t is not None and t.dtype != dt:
            raise TypeError("CSR must be int64 offsets and int32 sorted items")
    n, L = preds.shape
    nk = len(ks)
    dev = preds.device
    per_row = torch.empty((n, 4 * nk + 2), dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    cov = torch.zeros((num_items + 31) // 32, dtype=torch.int32, device=dev) if num_items > 0 else None
    karr = (ctypes.c_int32 * nk)(*ks)
    st = stream_of(preds)
    rows = lambda t: None if t is None else t.contiguous().to(torch.int64)  # noqa: E731
    gt_rows, ex_rows = rows(gt_rows), rows(ex_rows)
    call("rt_rank_metrics", ptr(preds), n, L, ptr(gt_offsets), ptr(gt_items), ptr(gt_rows), gt_offsets.numel() - 1,
         ptr(ex_offsets), ptr(ex_items), ptr(ex_rows), (ex_offsets.numel() - 1) if ex_offsets is not None else 0,
         karr, nk, num_items, ptr(per_row), ptr(valid), ptr(cov), st)
    summary = torch.empty(4 * nk + 4, dtype=torch.float64, device=dev)
    call("rt_rank_metrics_reduce", ptr(per_row), ptr(valid), n, 4 * nk + 2, ptr(cov), num_items, ptr(summary), st)
    return per_row, valid, summary


def list_metrics(preds: torch.Tensor, k_values, emb: Optional[torch.Tensor] = None,
                 info: Optional[torch.Tensor] = None, default_info: float = 0.0):
    """Intra-list diversity and novelty of device-resident rankings
    (src/evaluation/metrics.py:402-478) for every k in one pass
    (rt_list_metrics + rt_list_metrics_reduce). ``preds`` int64 [n, L] (-1 = no
    item); ``emb`` [n_emb, d] fp32 / fp16 / bf16 (a row stride is kept) and
    ``info`` fp64 [n_info] self-information (ids past it take ``default_info``)
    are each optional. Returns (div fp64 [n, n_k], div_valid int32 [n, n_k],
    nov_sum fp64 [n, n_k], nov_cnt int32 [n, n_k], summary fp64 [4, n_k] =
    diversity mean over valid rows, valid rows, novelty mean over entries,
    entries); a metric whose operand is None returns None tensors and zeros in
    the summary. Raises IndexError when a list holds an id >= n_emb (the kernel
    does not read it; costs a device sync)."""
    native.require_device(preds, emb, info, what="list_metrics")
    if emb is None and info is None:
        raise ValueError("list_metrics needs an embedding table, a self-information table, or both")
    if preds.dim() != 2:
        raise ValueError("preds must be [n_rows, list_len]")
    preds = preds.contiguous().to(torch.int64)
    ks = [int(k) for k in k_values]
    if not ks or len(ks) > native.RT_METRICS_MAX_K or sorted(set(ks)) != ks or ks[0] <= 0:
        raise ValueError(f"k_values must be 1..{native.RT_METRICS_MAX_K} ascending positive ints")
    n, L = preds.shape
    nk = len(ks)
    dev = preds.device
    div = valid = nov_sum = nov_cnt = oob = None
    dt, n_emb, d, ld = 0, 0, 0, 0
    if emb is not None:
        if emb.dim() != 2:
            raise ValueError("emb must be [n_emb, d]")
        dt = native.dtype_code(emb.dtype)
        n_emb, d = emb.shape
        if d < 1 or d > 1024 or (dt != native.RT_F32 and d % 8):
            raise ValueError(f"list_metrics: d = {d} unsupported for {emb.dtype} "
                             "(fp32: 1..1024; fp16 / bf16: a multiple of 8 up to 1024)")
        if n_emb > 1 and emb.stride(1) == 1 and emb.stride(0) >= d:
            ld = emb.stride(0)  # a row-strided view (a slice of the index's stored rows) is read in place
        else:
            emb, ld = emb.contiguous(), d
        div = torch.empty((n, nk), dtype=torch.float64, device=dev)
        valid = torch.empty((n, nk), dtype=torch.int32, device=dev)
        oob = torch.zeros(1, dtype=torch.int32, device=dev)
    if info is not None:
        if info.dim() != 1 or info.dtype != torch.float64:
            raise TypeError("info must be a 1-D float64 tensor")
        info = info.contiguous()
        nov_sum = torch.empty((n, nk), dtype=torch.float64, device=dev)
        nov_cnt = torch.empty((n, nk), dtype=torch.int32, device=dev)
    karr = (ctypes.c_int32 * nk)(*ks)
    st = stream_of(preds)
    gather_bytes = float(n) * L * d * (emb.element_size() if emb is not None else 0)
    with TIMER.region("list_metrics", bytes_=gather_bytes + 8.0 * n * L):
        call("rt_list_metrics", ptr(preds), n, L, ptr(emb), dt, n_emb, d, ld, ptr(info),
             info.numel() if info is not None else 0, float(default_info), karr, nk, ptr(div), ptr(valid),
             ptr(nov_sum), ptr(nov_cnt), ptr(oob), st)
        summary = torch.empty((4, nk), dtype=torch.float64, device=dev)
        call("rt_list_metrics_reduce", ptr(div), ptr(valid), ptr(nov_sum), ptr(nov_cnt), n, nk, ptr(summary), st)
    if oob is not None and int(oob.item()) != 0:
        raise IndexError(f"{int(oob.item())} ids out of range for an embedding table of {n_emb} rows")
    return div, valid, nov_sum, nov_cnt, summary


def sample_negatives(pos_offsets: torch.Tensor, pos_items: torch.Tensor, users: torch.Tensor, num_items: int,
                     num_neg: int, seed: int, seed_offset: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, num_neg] int64 negatives per row (rt_sample_negatives): distinct, uniform
    over the items user ``users[r]`` has not interacted with (CSR positives)."""
    native.require_device(pos_offsets, pos_items, users, what="sample_negatives")
    if pos_offsets.dtype != torch.int64 or pos_items.dtype != torch.int32:
        raise TypeError("CSR must be int64 offsets and int32 sorted items")
    users = users.contiguous().to(torch.int64)
    n = users.numel()
    if out is None:
        out = torch.empty((n, num_neg), dtype=torch.int64, device=users.device)
    with TIMER.region("sample_negatives", bytes_=8.0 * n * (num_neg + 1)):
        call("rt_sample_negatives", ptr(pos_offsets), ptr(pos_items), pos_offsets.numel() - 1, ptr(users), n,
             num_items, num_neg, seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_offset), ptr(out), stream_of(users))
    return out


def twotower_loss(u: torch.Tensor, p: torch.Tensor, q: Optional[torch.Tensor], temperature: float,
                  user_bias: Optional[torch.Tensor] = None, item_bias: Optional[torch.Tensor] = None,
                  explicit_weight: float = 0.7, in_batch_weight: float = 0.3, grad: bool = True):
    """Fused mixed loss (rt_twotower_loss_fwd_bwd / _fwd) on fp32, fp16 or bf16
    embeddings (widened to fp32 on load). Returns (loss fp64 [3] = (mixed,
    explicit, in-batch), du, dp, dq, d_user_bias, d_item_bias) — grads fp32 (None
    without ``grad``). q: [B*N, D] negatives (row i*N+j belongs to user i) or None."""
    native.require_device(u, p, what="twotower_loss")
    b, d = u.shape
    dt = native.dtype_code(u.dtype)
    if p.dtype != u.dtype or (q is not None and q.dtype != u.dtype):
        raise TypeError("u, p, q must share a dtype")
    u, p = u.contiguous(), p.contiguous()
    q = q.contiguous().reshape(-1, d) if q is not None else None
    n_neg = q.shape[0] // b if q is not None else 0
    dev = u.device
    loss = torch.zeros(3, dtype=torch.float64, device=dev)
    ws = workspace(dev, native.lib().rt_twotower_loss_workspace_bytes(b, d), "loss_k")
    f32 = dict(dtype=torch.float32, device=dev)
    st = stream_of(u)
    with TIMER.region("loss_fwd_bwd" if grad else "loss_fwd", flops=(6.0 if grad else 2.0) * b * b * d):
        if grad:
            du, dp = torch.empty((b, d), **f32), torch.empty((b, d), **f32)
            dq = torch.empty((q.shape[0], d), **f32) if q is not None else None
            dub = torch.zeros(1, **f32) if user_bias is not None else None
            dib = torch.zeros(1, **f32) if item_bias is not None else None
            call("rt_twotower_loss_fwd_bwd", ptr(u), ptr(p), ptr(q), dt, b, d, n_neg, 1.0 / temperature,
                 ptr(user_bias), ptr(item_bias), explicit_weight, in_batch_weight, ptr(loss), ptr(du), ptr(dp),
                 ptr(dq), ptr(dub), ptr(dib), ptr(ws), ws.numel(), st)
            return loss, du, dp, dq, dub, dib
        call("rt_twotower_loss_fwd", ptr(u), ptr(p), ptr(q), dt, b, d, n_neg, 1.0 / temperature, ptr(user_bias),
             ptr(item_bias), explicit_weight, in_batch_weight, ptr(loss), ptr(ws), ws.numel(), st)
        return loss, None, None, None, None, None


def inbatch_loss(u: torch.Tensor, p: torch.Tensor, temperature: float, label_offset: int = 0,
                 grad: bool = True):
    """In-batch CE of b local users against n_items in-batch items (label of user
    i = item label_offset + i) — rt_inbatch_loss_fwd_bwd. Returns (loss fp64 [3],
    du [b, D] fp32, dp [n_items, D] fp32); grads None without ``grad``."""
    native.require_device(u, p, what="inbatch_loss")
    if u.dtype != p.dtype:
        raise TypeError("u and p must share a dtype")
    u, p = u.contiguous(), p.contiguous()
    b, d = u.shape
    nx = p.shape[0]
    dev = u.device
    loss = torch.zeros(3, dtype=torch.float64, device=dev)
    ws = workspace(dev, native.lib().rt_inbatch_loss_workspace_bytes(b, nx, d), "inb")
    du = torch.empty((b, d), dtype=torch.float32, device=dev) if grad else None
    dp = torch.empty((nx, d), dtype=torch.float32, device=dev) if grad else None
    with TIMER.region("inbatch_loss", flops=(6.0 if grad else 2.0) * b * nx * d):
        call("rt_inbatch_loss_fwd_bwd", ptr(u), ptr(p), native.dtype_code(u.dtype), b, nx, d, label_offset,
             1.0 / temperature, ptr(loss), ptr(du), ptr(dp), ptr(ws), ws.numel(), stream_of(u))
    return loss, du, dp
