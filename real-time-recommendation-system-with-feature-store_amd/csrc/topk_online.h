// Online (small-batch) Flat-IP top-K: 1 <= nq <= 8 queries, k <= 128, bound by
// ONE streaming pass over the corpus instead of by query tiles. Serves the
// reference's serving path (faiss.IndexFlatIP.search with one user embedding,
// src/serving/retrieval.py:141-197 at Q = 1), where the GEMM-shaped scans of
// topk_impl.h fill one query tile and a quarter of the chip.
//
// Two launches:
//
// 1. flatip_online_scan: the grid is sized by ROWS (<= 512 blocks, 2 per CU);
//    block b owns the contiguous rows [b * rows_per_block, ...), so "lower id
//    wins" stays a property of position. A block = 4 waves; a wave walks
//    64-row groups of the block's 256-row tiles, ONE LANE PER ROW:
//      * a step moves 128 B of every row of the group (8 KiB per wave) with
//        coalesced 16-byte loads into registers, one step ahead of the compute
//        (8 waves per CU x 8 KiB = 64 KiB of loads in flight per CU), then into
//        the wave's LDS stage: rows padded to 144 B, so that the per-lane
//        ds_read_b128 of a row are conflict-free (the l2_renorm_kernel pattern);
//      * the queries sit in LDS as fp32 and are read as wave-uniform
//        (broadcast) ds_read_b128: no per-lane query loads;
//      * every (query, row) score is ONE lane's chain acc = fmaf(q[j], x[j], acc),
//        j ascending from 0 — the chain of oracle/flatip.c. 16-bit rows are
//        widened to fp32 first: every f16 x f16 and bf16 x bf16 product is exact
//        in fp32, so that form is the oracle's too. No dot / MFMA instructions:
//        the chain is what makes all three dtypes bit-exact. Measured at 1M x
//        128: at nq = 1 the scan runs at 62 % (f16) /
//        70 % (fp32) of the HBM pass; at nq = 8 it takes 134 / 153 us against a
//        32 / 64 us pass, bound by VALU issue plus the LDS broadcast of the
//        queries at two waves per SIMD, not by HBM.
//      * selection per (block, query): scores >= a running threshold are
//        appended to the query's LDS candidate buffer (one LDS atomic per wave
//        and query, positions by ballot); before a tile, a buffer above kRoom
//        (decided through the barrier that ended the tile before) is
//        compacted by the v4 radix compaction (threshold raised, never lowered).
//      * exclusions: a dense bitmap read per lane in the selection
//        (rt_flatip_topk_online), or CSR lists that the scan reads itself
//        (rt_flatip_topk_online_lists, the LISTS instantiation): cursors per
//        (query, source) in LDS, a 256-bit window per query built one tile
//        ahead, one wave-uniform LDS read per query in the selection. An
//        excluded row is never appended: nothing below changes.
//      * category filter (rt_flatip_topk_online_tags, the TAGS instantiation, on
//        top of LISTS): 64 bits of tags per row, one coalesced 8-byte load per
//        lane and tile issued a tile ahead with the row stream, tested against
//        the query's any_of / none_of masks in LDS. An ineligible row is never
//        appended either.
//      * the block then writes each query's best min(k, rows) entries, sorted,
//        as composite keys (score key << 32 | ~id; 0 = none) to
//        partials[query][rank][block] — rank-major, so that the finish reads
//        rank j of every block as one coalesced row.
// 2. flatip_online_finish: one block per query over the union of the block
//    lists. A list is sorted, so its entries at or above any bound are a prefix
//    of it, and the k-th best of the first ceil(k / blocks) ranks of every
//    list is a lower bound of the corpus-wide k-th: the finish walks the ranks
//    from 0, pools what is at or above the current bound, raises the bound by
//    a radix select on the composite key whenever the pool must shrink
//    (exact down to the id bits: massive ties), and stops at the first rank
//    where no list has an entry left. The <= 128 survivors take the unrolled
//    register sort; output in (score desc, id asc) order, (-FLT_MAX, -1) pads.
//    A second launch, not a last-block ticket: the kernel boundary gives
//    cross-XCD visibility of the partial lists for free.
#pragma once
#include "topk_impl.h"

namespace rt {
namespace topk {
namespace online {

constexpr int kMaxNq = 8;      // RT_ONLINE_MAX_NQ
constexpr int kMaxK = 128;     // RT_ONLINE_MAX_K
constexpr int kMaxBlocks = 512;  // 2 per CU; also the finish's threads (one per block list)
constexpr int kWavesS = 4;
constexpr int kThreads = 64 * kWavesS;
constexpr int kTileRows = 64 * kWavesS;  // rows a block scores between two compaction checks
constexpr int kMinRows = kTileRows;      // rows per block, at least
constexpr int kStepUnits = 8;            // 16-byte units of a row per step
constexpr int kRowStride = kStepUnits * 16 + 16;  // LDS bytes per staged row (one pad unit)
constexpr int kStageBytes = 64 * kRowStride;      // per wave

// Candidate buffer of one (block, query). The compaction check runs once per
// tile, before it; between two checks every row of the tile may pass, each
// appending one entry: the append budget is kTileRows. A buffer that passes
// the check holds <= kRoom entries, and a compaction leaves <= kRoom (its
// limit) of which the k best are kept.
constexpr int kCap = 448;
constexpr int kRoom = kCap - kTileRows;
static_assert(kRoom + kTileRows <= kCap, "online: a buffer at kRoom overflows before the next compaction check");
static_assert(kRoom >= kMaxK, "online: a compaction must be able to keep the k best");
static_assert(kMaxK <= v4::kFinishCap, "online: the block's list is sorted by the 128-entry register sort");

// Exclusion lists (rt_flatip_topk_online_lists): up to kMaxSrc CSR sources per
// call, query q skipping the union of its rows. The scan keeps, per (query,
// source), a cursor into the source's items; the (query, row) test of the
// selection reads a per-tile WINDOW of 256 bits per query in LDS, built one
// tile ahead from the cursors — never global memory.
constexpr int kMaxSrc = 2;  // RT_ONLINE_MAX_EXCL_SOURCES
constexpr int kWinWords = kTileRows / 32;

struct ListSrc {
    const int64_t* offsets;
    const int32_t* items;
    const int64_t* rows;
    int64_t n_rows;
};
template <bool LISTS>
struct ListArgs {};
template <>
struct ListArgs<true> {
    ListSrc src[kMaxSrc];
    int n;
};

// Tag filter (rt_flatip_topk_online_tags, rt_ivf_topk_tags): every item carries a
// 64-bit set of categories, a query an any_of and a none_of mask; a row is
// ELIGIBLE iff (any_of == 0 || (tags & any_of) != 0) && (tags & none_of) == 0.
// An ineligible row is never appended — one more term of `pass`, next to the
// exclusions. any_of / none_of may be null (all 0).
struct TagSrc {
    const uint64_t* item_tags;
    const uint64_t* any_of;
    const uint64_t* none_of;
};
template <bool TAGS>
struct TagArgs {};
template <>
struct TagArgs<true> : TagSrc {};

__device__ __forceinline__ bool tag_eligible(uint64_t tags, uint64_t any_of, uint64_t none_of) {
    return (any_of == 0ull || (tags & any_of) != 0ull) && (tags & none_of) == 0ull;
}

template <int NQ, bool LISTS = false, bool TAGS = false>
struct Lds {
    static constexpr int kStage = kWavesS * kStageBytes;
    static constexpr int kCand = NQ * kCap * static_cast<int>(sizeof(Cand));
    static constexpr int kQuery = NQ * 256 * 4;  // fp32 queries, d <= 256
    static constexpr int kHist = kWavesS * 256 * 4;
    // lists: cursor + end (int64) and next item (int32) per (query, source); two windows
    static constexpr int kPairs = NQ * kMaxSrc;
    static constexpr int kLists = LISTS ? kPairs * (8 + 8 + 4) + 2 * NQ * kWinWords * 4 : 0;
    // tags: any_of and none_of per query (uint64), behind the list state
    static constexpr int kTags = TAGS ? NQ * 16 : 0;
    static constexpr int kBytes = kStage + kCand + kQuery + kHist + kLists + kTags;
    static_assert(kLists % 8 == 0, "online: the list state holds 8-byte words");
    static_assert((kBytes - kTags) % 8 == 0, "online: the masks behind the list state are 8-byte words");
    static_assert(2 * (kBytes + 128) <= 163840, "online: two blocks per CU");
};

// The list state of one block in LDS. Query qi is OWNED by wave qi % kWavesS:
// only that wave reads or writes the query's cursors, and only it writes the
// query's windows; the other waves read a window after a block barrier.
struct ListState {
    int64_t* cur;    // [pairs] index of the first item not yet consumed
    int64_t* end;    // [pairs] end of the CSR row
    int32_t* next;   // [pairs] items[cur] (a hint: INT32_MAX when the row is consumed)
    uint32_t* win;   // [2][NQ][kWinWords]: bit r of window t & 1 = row r of tile t is excluded
};

// Prologue, per wave: 16-lane group g serves (query wave + 4 (g >> 1), source
// g & 1): the CSR row's range, then the first item >= row_begin by a 17-ary
// search (one probe per lane and round: 166 items take two dependent loads).
template <int NQ>
__device__ __forceinline__ void lists_begin(const ListArgs<true>& la, const ListState& ls, int nq, int64_t row_begin) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, gl = lane & 15;
    const int qi = wave + kWavesS * (g >> 1), s = g & 1;
    const bool mine = qi < nq && qi < NQ && s < la.n;
    const int64_t* offsets = s ? la.src[1].offsets : la.src[0].offsets;
    const int32_t* items = s ? la.src[1].items : la.src[0].items;
    const int64_t* rows = s ? la.src[1].rows : la.src[0].rows;
    const int64_t n_rows = s ? la.src[1].n_rows : la.src[0].n_rows;
    int64_t lo = 0, hi = 0;
    if (mine) {
        const int64_t r = rows ? rows[qi] : static_cast<int64_t>(qi);
        if (r >= 0 && r < n_rows) {
            lo = offsets[r];
            hi = offsets[r + 1];
            if (hi < lo) hi = lo;
        }
    }
    const int64_t row_last = hi;
    // invariant: every item before lo is < row_begin; the item at hi (or none) is not
    bool act = hi > lo;
    while (__any(act)) {
        const int64_t step = (hi - lo + 15) >> 4;
        const int64_t idx = lo + (gl + 1) * step - 1;
        const bool in = act && idx < hi;
        const int32_t v = in ? items[idx] : 0;
        const uint64_t bm = __ballot(in && static_cast<int64_t>(v) < row_begin);
        const int c = __popc(static_cast<uint32_t>(bm >> (g * 16)) & 0xFFFFu);
        if (act) {
            const int64_t a = lo + c * step, b = lo + (c + 1) * step - 1;
            lo = a < hi ? a : hi;
            hi = b < hi ? b : hi;
            act = hi > lo;
        }
    }
    if (qi < NQ && s < kMaxSrc && gl == 0) {
        const int p = qi * kMaxSrc + s;
        ls.cur[p] = lo;
        ls.end[p] = row_last;
        ls.next[p] = (mine && lo < row_last) ? items[lo] : INT32_MAX;
    }
}

// Window of tile tt for the queries this wave owns: the items of every source
// in [tile_lo, tile_hi), consumed from the cursors. A row's items ascend, so
// they are a run from the cursor; a lane takes one item per round, a round
// consumes up to 64, and a run of any length is consumed in further rounds.
// `next` keeps the common case — no item of the row in this tile — free of
// any global load. Bits are set only for tile_lo <= item < tile_hi: a row that
// does not ascend excludes the wrong rows, but writes inside its window.
template <int NQ>
__device__ __forceinline__ void lists_window(const ListArgs<true>& la, const ListState& ls, int nq, int tt,
                                             int64_t row_begin, int64_t row_end) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile_lo = row_begin + static_cast<int64_t>(tt) * kTileRows;
    const int64_t tile_hi = (tile_lo + kTileRows) < row_end ? (tile_lo + kTileRows) : row_end;
    for (int qi = wave; qi < nq && qi < NQ; qi += kWavesS) {
        uint32_t* const w = ls.win + ((tt & 1) * NQ + qi) * kWinWords;
        if (lane < kWinWords) w[lane] = 0u;
        wave_lds_sync();
#pragma unroll
        for (int s = 0; s < kMaxSrc; ++s) {
            if (s >= la.n) break;  // block-uniform
            const int p = qi * kMaxSrc + s;
            if (static_cast<int64_t>(ls.next[p]) >= tile_hi) continue;  // wave-uniform
            const int32_t* items = la.src[s].items;
            int64_t c = ls.cur[p];
            const int64_t e = ls.end[p];
            int32_t nv = INT32_MAX;
            for (;;) {
                const int64_t idx = c + lane;
                const int32_t v = idx < e ? items[idx] : INT32_MAX;
                const bool take = static_cast<int64_t>(v) < tile_hi;  // INT32_MAX: only when idx < e
                if (take && idx < e && v >= tile_lo) {
                    const uint32_t r = static_cast<uint32_t>(v - tile_lo);
                    atomicOr(&w[r >> 5], 1u << (r & 31u));
                }
                const int adv = __popcll(__ballot(take && idx < e));
                c += adv;
                if (adv < 64) {
                    nv = __shfl(v, adv, 64);  // the first item not consumed (INT32_MAX: none)
                    break;
                }
            }
            wave_lds_sync();
            if (lane == 0) {
                ls.cur[p] = c;
                ls.next[p] = nv;
            }
        }
        wave_lds_sync();
    }
}

__device__ __forceinline__ void widen(const uint4& v, float (&x)[4], float) {
    x[0] = __uint_as_float(v.x); x[1] = __uint_as_float(v.y);
    x[2] = __uint_as_float(v.z); x[3] = __uint_as_float(v.w);
}
__device__ __forceinline__ void widen(const uint4& v, float (&x)[8], __half) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = bits_f16_to_f32(static_cast<uint16_t>(w[i] & 0xFFFFu));
        x[2 * i + 1] = bits_f16_to_f32(static_cast<uint16_t>(w[i] >> 16));
    }
}
__device__ __forceinline__ void widen(const uint4& v, float (&x)[8], __hip_bfloat16) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = __uint_as_float(w[i] << 16);
        x[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
    }
}

// ---- the row stream both scans share (flatip_online_scan; ivf_scan, ivf.hip) ----
// A block's row window: the stored rows [row_begin, row_end) of X, `units`
// 16-byte units each, walked in `tiles` 256-row tiles of `steps` column steps.
struct RowWindow {
    const char* X;
    int64_t row_begin, row_end, row_bytes;
    int units, steps, tiles;
};

// step (tile t, column step c) of this wave: slot i of lane l is unit
// c * 8 + (f & 7) of group row f >> 3, f = 64 i + l
__device__ __forceinline__ void load_step(uint4 (&R)[kStepUnits], const RowWindow& w, int t, int c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g0 = w.row_begin + static_cast<int64_t>(t) * kTileRows + wave * 64;
#pragma unroll
    for (int i = 0; i < kStepUnits; ++i) {
        const int f = i * 64 + lane;
        const int u = c * kStepUnits + (f & 7);
        const int64_t row = g0 + (f >> 3);
        R[i] = make_uint4(0u, 0u, 0u, 0u);
        if (t < w.tiles && u < w.units && row < w.row_end)
            R[i] = *reinterpret_cast<const uint4*>(w.X + row * w.row_bytes + static_cast<int64_t>(u) * 16);
    }
}

// Staged score chain: acc[qi] = the score of query qi (fp32 in LDS at
// qs + qi * d) against this lane's row of tile t — the wave's 64-row group,
// lane = row. R holds the tile's first step on entry (load_step) and the next
// tile's first step on return: every step is loaded one ahead of its compute.
template <typename T, int NQ>
__device__ __forceinline__ void score_tile(uint4 (&R)[kStepUnits], const RowWindow& w, int t, char* stage,
                                           const float* qs, int d, float (&acc)[NQ]) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));  // elements per 16-byte unit
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) acc[qi] = 0.f;
    for (int c = 0; c < w.steps; ++c) {
#pragma unroll
        for (int i = 0; i < kStepUnits; ++i) {
            const int f = i * 64 + lane;
            *reinterpret_cast<uint4*>(stage + (f >> 3) * kRowStride + (f & 7) * 16) = R[i];
        }
        if (c + 1 < w.steps) load_step(R, w, t, c + 1);
        else load_step(R, w, t + 1, 0);
        wave_lds_sync();
        const int nu = (w.units - c * kStepUnits) < kStepUnits ? (w.units - c * kStepUnits) : kStepUnits;
#pragma unroll
        for (int u = 0; u < kStepUnits; ++u) {
            if (u >= nu) break;  // wave-uniform
            const uint4 xv = *reinterpret_cast<const uint4*>(stage + lane * kRowStride + u * 16);
            float x[EPU];
            widen(xv, x, T());
            const int j0 = (c * kStepUnits + u) * EPU;
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
                for (int h = 0; h < EPU / 4; ++h) {
                    const float4 qv = *reinterpret_cast<const float4*>(qs + qi * d + j0 + 4 * h);
                    acc[qi] = __builtin_fmaf(qv.x, x[4 * h], acc[qi]);
                    acc[qi] = __builtin_fmaf(qv.y, x[4 * h + 1], acc[qi]);
                    acc[qi] = __builtin_fmaf(qv.z, x[4 * h + 2], acc[qi]);
                    acc[qi] = __builtin_fmaf(qv.w, x[4 * h + 3], acc[qi]);
                }
            }
        }
        wave_lds_sync();  // the stage is rewritten by the next step
    }
}

// Append (s, id) of the lanes with `pass` to one query's candidate buffer: one
// LDS atomic per wave, positions by ballot rank. `pass` comes from registers
// and LDS only — a per-lane global load between the scores and the ballot
// would be waited for with every load before it drained, the next tile's
// prefetch included. Returns whether this append took the buffer above kRoom.
// The position is < kCap by the append budget; GUARD tests it all the same,
// for a caller whose ids may repeat (equal keys, which no compaction can tell
// apart, so a compaction may leave more than kRoom).
template <bool GUARD>
__device__ __forceinline__ int append(bool pass, int* cnt, Cand* buf, float s, uint32_t id) {
    const uint64_t bm = __ballot(pass);
    if (!bm) return 0;
    int base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(cnt, __popcll(bm));
    base = __shfl(base, 0, 64);
    const int at = base + ballot_rank(bm);
    if (pass && (!GUARD || at < kCap)) buf[at] = Cand{s, id};
    return (base + __popcll(bm)) > kRoom ? 1 : 0;
}

// wave: the block's list of one query — the k best of buf[0, n), sorted, as
// composite keys to out[rank * stride], 0 for none
__device__ __forceinline__ void write_block_list(Cand* buf, int n, int k, uint32_t* hist, uint64_t* out,
                                                 int64_t stride) {
    const int lane = threadIdx.x & 63;
    if (n > v4::kFinishCap) {
        float th = 0.f;
        v4::compact_stream(buf, n, k, v4::kFinishCap, hist, th);
    }
    wave_lds_sync();
    float s[2];
    uint32_t id[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = lane * 2 + j;
        const Cand cd = r < n ? buf[r] : Cand{-INFINITY, kEmptyId};
        s[j] = cd.s;
        id[j] = cd.i;
    }
    wave_sort_regs2(s, id);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = lane * 2 + j;
        if (r < k) out[r * stride] = id[j] != kEmptyId ? v4::ckey(Cand{s[j], id[j]}) : 0ull;
    }
}

// LISTS: the exclusions are `la`'s CSR lists (excl is not read); otherwise the
// optional dense bitmap `excl`. TAGS: `ta`'s tag filter on top (tags indexed by
// row): the lane's 8 bytes are one coalesced load per tile, issued one tile
// ahead in front of the tile's row stream — older than every load the tile
// waits for, so the selection finds them in registers; the masks sit in LDS.
template <typename T, int NQ, bool LISTS, bool TAGS = false>
__global__ __launch_bounds__(kThreads, 2) void flatip_online_scan(
    const T* __restrict__ Q, int nq, const char* __restrict__ X, int64_t nx, int d, int k,
    const uint32_t* __restrict__ excl, int64_t excl_words, int64_t rows_per_block, int blocks,
    uint64_t* __restrict__ partials, const ListArgs<LISTS> la, const TagArgs<TAGS> ta) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));
    __shared__ __attribute__((aligned(16))) char lds[Lds<NQ, LISTS, TAGS>::kBytes];
    __shared__ int cnt[kMaxNq];
    __shared__ float thr[kMaxNq];
    char* const stage = lds + (threadIdx.x >> 6) * kStageBytes;
    Cand* const cand = reinterpret_cast<Cand*>(lds + Lds<NQ>::kStage);
    float* const qs = reinterpret_cast<float*>(lds + Lds<NQ>::kStage + Lds<NQ>::kCand);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + Lds<NQ>::kStage + Lds<NQ>::kCand + Lds<NQ>::kQuery) +
                           (threadIdx.x >> 6) * 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    RowWindow w;
    w.X = X;
    w.row_begin = static_cast<int64_t>(b) * rows_per_block;
    w.row_end = (w.row_begin + rows_per_block) < nx ? (w.row_begin + rows_per_block) : nx;
    w.units = d / EPU;
    w.row_bytes = static_cast<int64_t>(w.units) * 16;
    w.steps = (w.units + kStepUnits - 1) / kStepUnits;
    w.tiles = static_cast<int>((w.row_end - w.row_begin + kTileRows - 1) / kTileRows);

    // queries as fp32 (padding queries: zeros), counters, thresholds
    for (int e = threadIdx.x; e < NQ * d; e += kThreads) {
        const int qi = e / d;
        qs[e] = qi < nq ? to_f32(Q[e]) : 0.f;
    }
    if (threadIdx.x < kMaxNq) {
        cnt[threadIdx.x] = 0;
        thr[threadIdx.x] = -INFINITY;
    }

    uint4 R[kStepUnits];
    load_step(R, w, 0, 0);
    // TAGS: the masks of query qi at tmask[2 qi], tmask[2 qi + 1]; tg_next = the
    // tags of this lane's row of the tile after the one being scored
    uint64_t* const tmask = reinterpret_cast<uint64_t*>(lds + Lds<NQ, LISTS>::kBytes);
    uint64_t tg_next = 0ull;
    if constexpr (TAGS) {
        if (threadIdx.x < 2 * NQ) {
            const int qi = threadIdx.x >> 1;
            const uint64_t* m = (threadIdx.x & 1) ? ta.none_of : ta.any_of;
            tmask[threadIdx.x] = (m && qi < nq) ? m[qi] : 0ull;
        }
        const int64_t row0 = w.row_begin + threadIdx.x;
        if (row0 < w.row_end) tg_next = ta.item_tags[row0];
    }
    ListState ls{};
    if constexpr (LISTS) {
        // while the first step is in flight: the cursors and tile 0's window
        char* const base = lds + Lds<NQ>::kBytes;
        constexpr int P = Lds<NQ, true>::kPairs;
        ls.cur = reinterpret_cast<int64_t*>(base);
        ls.end = ls.cur + P;
        ls.next = reinterpret_cast<int32_t*>(ls.end + P);
        ls.win = reinterpret_cast<uint32_t*>(ls.next + P);
        lists_begin<NQ>(la, ls, nq, w.row_begin);
        wave_lds_sync();
        lists_window<NQ>(la, ls, nq, 0, w.row_begin, w.row_end);
    }
    __syncthreads();

    // `over`: some buffer holds more than kRoom entries. The decision is taken
    // THROUGH the barrier that ends a tile (__syncthreads_or over what every
    // wave's own append returned: the last append to a query saw base + n =
    // its final count), never by reading cnt, which waves already in the next
    // tile's selection may be raising: so the branch below, which holds a
    // barrier, is block-uniform, and the check sees every append of the tiles
    // before and none of this one.
    int over = 0;
    for (int t = 0; t < w.tiles; ++t) {
        if (over) {
            for (int qi = wave; qi < NQ; qi += kWavesS) {
                int n = cnt[qi];
                if (n > kRoom) {
                    float th = thr[qi];
                    v4::compact_stream(cand + qi * kCap, n, k, kRoom, hist, th);
                    if (lane == 0) {
                        cnt[qi] = n;
                        thr[qi] = th;
                    }
                }
            }
            __syncthreads();
        }
        float th[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) th[qi] = thr[qi];

        const int64_t row = w.row_begin + static_cast<int64_t>(t) * kTileRows + wave * 64 + lane;
        const uint64_t tg = tg_next;
        if constexpr (TAGS) {
            tg_next = 0ull;
            if (row + kTileRows < w.row_end) tg_next = ta.item_tags[row + kTileRows];
        }

        float acc[NQ];
        score_tile<T, NQ>(R, w, t, stage, qs, d, acc);

        // ---- selection: appends of at most one entry per row and query ----
        const bool valid = row < w.row_end;
        int mine_over = 0;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            if (qi < nq) {
                bool pass = valid && acc[qi] >= th[qi];
                if constexpr (LISTS) {
                    // bit wave * 64 + lane of the query's window: one wave-uniform
                    // 8-byte LDS read
                    const uint64_t wbits = *reinterpret_cast<const uint64_t*>(
                        ls.win + ((t & 1) * NQ + qi) * kWinWords + wave * 2);
                    pass = pass && ((wbits >> lane) & 1ull) == 0ull;
                } else if (excl && pass)
                    // the per-lane global load `append` warns of: a call with
                    // exclude_bits loses the one-step-ahead streaming
                    pass = ((excl[qi * excl_words + (row >> 5)] >> (row & 31)) & 1u) == 0u;
                if constexpr (TAGS)  // two wave-uniform 8-byte LDS reads
                    pass = pass && tag_eligible(tg, tmask[2 * qi], tmask[2 * qi + 1]);
                mine_over |= append<false>(pass, &cnt[qi], cand + qi * kCap, acc[qi], static_cast<uint32_t>(row));
            }
        }
        if constexpr (LISTS) {
            // the next tile's window, into the buffer whose last readers (tile t - 1's
            // selection) are behind the barrier that ended that tile; the barrier
            // below publishes it
            if (t + 1 < w.tiles) lists_window<NQ>(la, ls, nq, t + 1, w.row_begin, w.row_end);
        }
        over = __syncthreads_or(mine_over);
    }

    // ---- the block's list per query: partials[query][rank][block] ----
    for (int qi = wave; qi < nq; qi += kWavesS)
        write_block_list(cand + qi * kCap, cnt[qi], k, hist, partials + (static_cast<int64_t>(qi) * k) * blocks + b,
                         blocks);
}

// ---- finish ----
constexpr int kPool = 4096;  // pooled composite keys (LDS); a rank adds <= kMaxBlocks
static_assert(v4::kFinishCap + kMaxBlocks <= kPool, "online finish: a pool after a select takes one more rank");

// wave 0: the pool keeps, in place, its entries in the radix bucket of its
// k-th best (<= 128 of them, the k best among them); bound = the bucket's floor
__device__ __forceinline__ void pool_select(uint64_t* pool, int& n, int k, uint32_t* hist, uint64_t& bound) {
    const int lane = threadIdx.x & 63;
    const int n_in = n;
    auto each = [&](auto&& fn) {
        for (int i = lane; i < n_in; i += 64) fn(pool[i]);
    };
    uint64_t prefix = 0;
    int shift = 64, kept = n_in;
    v4::radix_prefix(each, k, v4::kFinishCap, hist, prefix, shift, kept);
    const uint64_t pmask = v4::prefix_mask(shift);
    int m = 0;
    for (int i0 = 0; i0 < n_in; i0 += 64) {
        const int i = i0 + lane;
        uint64_t key = 0ull;
        bool take = false;
        if (i < n_in) {
            key = pool[i];
            take = (key & pmask) >= prefix;
        }
        const uint64_t bm = __ballot(take);
        const int pos = m + ballot_rank(bm);
        wave_lds_sync();
        if (take) pool[pos] = key;  // pos <= i: every lane read its entry before any lane writes
        m += __popcll(bm);
    }
    wave_lds_sync();
    n = m;
    bound = prefix;
}

static __global__ __launch_bounds__(kMaxBlocks) void flatip_online_finish(const uint64_t* __restrict__ partials, int blocks,
                                                                   int k, float* __restrict__ out_s,
                                                                   int64_t* __restrict__ out_i, int64_t id_offset) {
    __shared__ __attribute__((aligned(16))) uint64_t pool[kPool];
    __shared__ __attribute__((aligned(16))) uint32_t hist[256];
    __shared__ __attribute__((aligned(16))) Cand keep[v4::kFinishCap];
    __shared__ int pn;
    __shared__ uint64_t pbound;
    const int t = threadIdx.x, lane = t & 63;
    const int q = blockIdx.x;
    const bool active = t < blocks;
    const uint64_t* mine = partials + static_cast<int64_t>(q) * k * blocks + t;
    if (t == 0) {
        pn = 0;
        pbound = 0ull;
    }
    __syncthreads();
    const int first = blocks > 0 ? (k + blocks - 1) / blocks : 1;  // ranks that hold >= k entries of full lists
    uint64_t next = active ? mine[0] : 0ull;
    for (int j = 0; j < k; ++j) {
        const uint64_t cur = next;
        if (active && j + 1 < k) next = mine[static_cast<int64_t>(j + 1) * blocks];
        const uint64_t bound = pbound;
        const bool take = cur != 0ull && cur >= bound;
        const uint64_t bm = __ballot(take);
        if (bm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&pn, __popcll(bm));
            base = __shfl(base, 0, 64);
            const int pos = base + ballot_rank(bm);
            if (take) pool[pos] = cur;
        }
        // no list has an entry at this rank at or above the bound: none has one
        // at a later rank either (the lists are sorted, the bound only rises)
        if (!__syncthreads_or(take ? 1 : 0)) break;
        const int n_now = pn;
        // the first bound as soon as the ranks walked hold k entries of full
        // lists; later ones only when the pool could not take another rank
        const bool select = n_now > v4::kFinishCap &&
                            ((bound == 0ull && j + 1 >= first) || n_now + kMaxBlocks > kPool);
        if (select) {  // block-uniform
            if (t < 64) {
                int n = n_now;
                uint64_t bd = 0ull;
                pool_select(pool, n, k, hist, bd);
                if (lane == 0) {
                    pn = n;
                    pbound = bd;
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (t >= 64) return;
    int n = pn;
    if (n > v4::kFinishCap) {
        uint64_t bd = 0ull;
        pool_select(pool, n, k, hist, bd);
    }
    for (int r = lane; r < n; r += 64) {
        const uint64_t key = pool[r];
        keep[r] = Cand{v2::okey_inv(static_cast<uint32_t>(key >> 32)), ~static_cast<uint32_t>(key)};
    }
    wave_lds_sync();
    v4::finish_sort<2>(keep, n, k, out_s + static_cast<int64_t>(q) * k, out_i + static_cast<int64_t>(q) * k,
                       id_offset);
}

// one block per query over the `lists` sorted partial lists of a scan (0: none, every slot a pad)
inline int launch_finish(const uint64_t* partials, int lists, int k, float* out_s, int64_t* out_i, int64_t id_offset,
                         int64_t nq, hipStream_t st) {
    hipLaunchKernelGGL(flatip_online_finish, dim3(static_cast<unsigned>(nq)), dim3(kMaxBlocks), 0, st, partials, lists,
                       k, out_s, out_i, id_offset);
    return check_launch("flatip_online_finish");
}

// rows the staged chain takes: whole 16-byte units, d <= 256 (the queries' LDS)
inline bool shape_ok(int d, int dtype) {
    return dtype == RT_F32 ? (d % 4 == 0 && d <= 256) : (d % 8 == 0 && d <= 256);
}

struct OnlinePlan {
    int blocks;
    int64_t rows_per_block;
};
// rows alone size the grid: as many blocks as give each >= kMinRows rows, <= kMaxBlocks
inline OnlinePlan make_plan(int64_t nx) {
    OnlinePlan p{1, kMinRows};
    if (nx <= 0) return p;
    int64_t rpb = (nx + kMaxBlocks - 1) / kMaxBlocks;
    if (rpb < kMinRows) rpb = kMinRows;
    p.rows_per_block = rpb;
    p.blocks = static_cast<int>((nx + rpb - 1) / rpb);
    return p;
}
inline size_t workspace_bytes(int64_t nq, int k, const OnlinePlan& p) {
    return static_cast<size_t>(nq) * k * p.blocks * sizeof(uint64_t);
}

template <typename T, bool LISTS = false, bool TAGS = false>
int launch_scan(const void* Q, int nq, const void* X, int64_t nx, int d, int k, const uint32_t* excl,
                int64_t excl_words, const OnlinePlan& p, uint64_t* partials, hipStream_t st,
                const ListArgs<LISTS>& la = ListArgs<LISTS>(), const TagArgs<TAGS>& ta = TagArgs<TAGS>()) {
    const dim3 grid(static_cast<unsigned>(p.blocks)), block(kThreads);
    const T* q = static_cast<const T*>(Q);
    const char* x = static_cast<const char*>(X);
#define RT_ONLINE_LAUNCH(NQ)                                                                                       \
    hipLaunchKernelGGL((flatip_online_scan<T, NQ, LISTS, TAGS>), grid, block, 0, st, q, nq, x, nx, d, k, excl,     \
                       excl_words, p.rows_per_block, p.blocks, partials, la, ta)
    if (nq <= 1) RT_ONLINE_LAUNCH(1);
    else if (nq <= 2) RT_ONLINE_LAUNCH(2);
    else if (nq <= 4) RT_ONLINE_LAUNCH(4);
    else RT_ONLINE_LAUNCH(8);
#undef RT_ONLINE_LAUNCH
    return check_launch("flatip_online_scan");
}

}  // namespace online
}  // namespace topk
}  // namespace rt
