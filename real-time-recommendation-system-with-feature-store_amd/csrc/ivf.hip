// IVF-Flat: the probed-list scan (rt_ivf_topk) and the centroid update of one
// Lloyd step (rt_segment_mean_f32). Serves the reference's default index,
// faiss.index_factory(d, "IVF1024,Flat") searched with nprobe = 20
// (src/serving/retrieval.py:60-62, 101-133, 141-197).
//
// rt_ivf_topk, two launches:
//
// 1. ivf_scan: grid (probe x chunk, query). The corpus is stored
//    list-contiguous; block (p, c) of query q reads probes[q][p], clamps chunk c
//    of that list to [off[l], off[l + 1]) and to [0, nx), and leaves at once
//    (its partial list all "none") when nothing is left. Over that row window it
//    runs the online scan's row stream for ONE query — online::score_tile,
//    online::append and online::write_block_list (topk_online.h) are the same
//    code, so scores are bit-identical to the Flat index's. What differs:
//      * the id: a candidate carries the ORIGINAL corpus position row_pos[row],
//        the exclusion bitmap is indexed by it, and the composite key (score
//        key << 32 | ~position) holds the tie rule — the storage order does
//        not reach the result;
//      * the compaction: rows therefore do NOT arrive in id order, and the
//        filter threshold after a compaction is the lowest score kept (an
//        equal later score may still win on its position), never the
//        "strictly above" of compact_stream's tie case;
//      * the append is guarded: a row_pos that repeats positions gives equal
//        keys, of which a compaction may keep more than its limit.
// 2. flatip_online_finish (topk_online.h, unchanged): one block per query over
//    the nprobe x chunks <= 512 sorted partial lists.
//
// The grid depends on host arguments only (nq, nprobe, max_list_rows): no host
// read, stream-ordered, capturable.
//
// rt_ivf_topk_lists: the same two launches, the scan's LISTS instantiation. The
// exclusions are CSR lists of ORIGINAL positions instead of the bitmap. Stored
// rows do not arrive in position order (row_pos is any permutation), so the
// Flat scan's cursors and windows do not apply: a lane whose row passed the
// range and threshold tests looks its position up by a lower-bound binary
// search in its query's CSR row of every source. The block resolves those rows
// once, in its prologue, and copies them into LDS when together they fit
// kListCap entries (else the search reads `items` in global memory): one
// search routine over a generic pointer serves both.
//
// rt_ivf_topk_tags: the LISTS scan's TAGS instantiation (any number of sources,
// none included). item_tags is indexed by ORIGINAL position, so the lists'
// layout and rt_ivf_lists_update know nothing of it: the lane gathers
// item_tags[pos] as soon as it holds pos, in flight under the scores, and only
// for a pos inside [0, n_pos). Eligibility is one more term of `pass`.
//
// rt_ivf_topk_lens / rt_ivf_topk_lists_lens: the same kernels over lists stored
// with slack (ivf_mutate.hip). Two more operands: list_len (the live rows of a
// list are the first list_len[l] of its capacity) and n_pos (positions are valid
// in [0, n_pos), where the other two entry points use nx). The grid is sized by
// the largest CAPACITY, a host argument, so a captured call sees lists that
// changed in place. The other two entry points pass list_len = nullptr and
// n_pos = nx: the window and the range test they had.
#include "topk_online.h"

namespace rt {
namespace topk {
namespace ivf {

namespace on = rt::topk::online;

constexpr int kMaxProbe = 128;                // RT_IVF_MAX_NPROBE
constexpr int kMaxLists = on::kMaxBlocks;     // partial lists per query the finish takes (one thread each)
constexpr int64_t kMaxNq = 65535;             // grid.y
static_assert(kMaxProbe <= kMaxLists, "ivf: one partial list per probe at least");

struct Plan {
    int chunks;              // per probed list
    int64_t rows_per_chunk;  // a multiple of the scan's 256-row tile
};

// Smallest chunks (>= min_tiles tiles) that keep nprobe x chunks within the
// finish's 512 lists: at nq = 1 the blocks of a call are all the parallelism
// there is (20 probes of ~1,000 rows = 80 blocks of one tile, not 20).
inline Plan make_plan(int nprobe, int64_t max_list_rows, int min_tiles) {
    const int64_t tile = on::kTileRows;
    const int64_t mlr = max_list_rows > 0 ? max_list_rows : 1;
    const int64_t cap = kMaxLists / (nprobe > 0 ? nprobe : 1);  // >= 4
    int64_t tiles = (mlr + tile - 1) / tile;
    int64_t tpc = (tiles + cap - 1) / cap;  // tiles per chunk
    if (tpc < min_tiles) tpc = min_tiles;
    Plan p;
    p.rows_per_chunk = tpc * tile;
    p.chunks = static_cast<int>((mlr + p.rows_per_chunk - 1) / p.rows_per_chunk);
    return p;
}

// wave: compact one candidate buffer; thr = the lowest score kept
__device__ __forceinline__ void compact_keep_ties(Cand* buf, int& n, int k, int limit, uint32_t* hist, float& thr) {
    const int lane = threadIdx.x & 63;
    float unused = 0.f;
    v4::compact_stream(buf, n, k, limit, hist, unused);
    wave_lds_sync();
    float lo = INFINITY;
    for (int i = lane; i < n; i += 64) lo = fminf(lo, buf[i].s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    thr = lo;
}

// ---- exclusion lists (the LISTS instantiation) ----
// The staged lists take what two blocks per CU leave of the LDS next to the
// scan's own Lds<1>: (163,840 / 2 - 128) - 45,568 - 384 = 35,840 B = 8,960
// positions for the query's CSR rows of all sources together. The 384 B stand
// for what the block holds outside `lds`: cnt and thr, the 256 B scratch of the
// block-wide reduction behind __syncthreads_or, and alignment.
constexpr int kLdsPerBlock = 163840 / 2 - 128;
constexpr int kListSlack = 384;
constexpr int kListBytes = ((kLdsPerBlock - on::Lds<1>::kBytes - kListSlack) / 16) * 16;
constexpr int kListCap = kListBytes / 4;
static_assert(kListBytes > 0 && kListBytes % 16 == 0, "ivf: the staged lists follow the scan's 16-byte aligned LDS");
static_assert(2 * (on::Lds<1>::kBytes + kListBytes + kListSlack + 128) <= 163840, "ivf: two blocks per CU");

// Whether items[lo, hi) (ascending; LDS or global) holds `pos`, for the lanes
// with `act`: a lower bound by bisection. Every lane of the wave calls it; the
// loop runs until no lane has a range left (wave-uniform trip count, no
// barrier inside). Every read is at an index in [lo, hi), whatever the items
// hold: a row that does not ascend gives a wrong answer, nothing worse.
__device__ __forceinline__ bool list_has(const int32_t* items, int64_t lo, int64_t hi, int32_t pos, bool act) {
    int64_t a = lo, b = act ? hi : lo;
    while (__any(a < b)) {
        if (a < b) {
            const int64_t mid = a + ((b - a) >> 1);
            if (items[mid] < pos) a = mid + 1;
            else b = mid;
        }
    }
    return act && a < hi && items[a] == pos;
}

// LISTS: the exclusions are `la`'s CSR lists (excl is not read); otherwise the
// optional dense bitmap `excl`. TAGS: `ta`'s tag filter on top.
template <typename T, bool LISTS, bool TAGS = false>
__global__ __launch_bounds__(on::kThreads, 2) void ivf_scan(
    const T* __restrict__ Q, const char* __restrict__ X, int64_t nx, int d, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int64_t* __restrict__ list_len, int64_t n_pos,
    const int32_t* __restrict__ row_pos, const int64_t* __restrict__ probes, int nprobe, int chunks,
    int64_t rows_per_chunk,
    const uint32_t* __restrict__ excl, int64_t excl_words, uint64_t* __restrict__ partials,
    const on::ListArgs<LISTS> la, const on::TagArgs<TAGS> ta) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));
    constexpr int kThreads = on::kThreads, kTileRows = on::kTileRows, kStepUnits = on::kStepUnits;
    using L = on::Lds<1>;
    __shared__ __attribute__((aligned(16))) char lds[L::kBytes + (LISTS ? kListBytes : 0)];
    __shared__ int cnt;
    __shared__ float thr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lists = nprobe * chunks;
    const int lb = blockIdx.x, q = blockIdx.y;
    const int p = lb / chunks, c = lb - p * chunks;
    uint64_t* const out = partials + static_cast<int64_t>(q) * k * lists + lb;  // [q][rank][lb]

    // the chunk, clamped to the list and to the corpus
    on::RowWindow w;
    w.X = X;
    w.row_begin = w.row_end = 0;
    const int64_t l = probes[static_cast<int64_t>(q) * nprobe + p];
    if (l >= 0 && l < nlist) {
        int64_t lo = list_offsets[l], hi = list_offsets[l + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > nx ? nx : hi;
        if (list_len && lo < hi) {  // lists with slack: the first list_len[l] rows of the capacity
            const int64_t live = list_len[l];
            hi = live <= 0 ? lo : (live < hi - lo ? lo + live : hi);
        }
        if (lo < hi) {
            const int64_t len = hi - lo, first = static_cast<int64_t>(c) * rows_per_chunk;
            if (first < len) {
                w.row_begin = lo + first;
                w.row_end = (first + rows_per_chunk) < len ? (w.row_begin + rows_per_chunk) : hi;
            }
        }
    }
    if (w.row_end <= w.row_begin) {  // block-uniform
        for (int r = threadIdx.x; r < k; r += kThreads) out[static_cast<int64_t>(r) * lists] = 0ull;
        return;
    }

    char* const stage = lds + wave * on::kStageBytes;
    Cand* const cand = reinterpret_cast<Cand*>(lds + L::kStage);
    float* const qs = reinterpret_cast<float*>(lds + L::kStage + L::kCand);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + L::kStage + L::kCand + L::kQuery) + wave * 256;
    w.units = d / EPU;
    w.row_bytes = static_cast<int64_t>(w.units) * 16;
    w.steps = (w.units + kStepUnits - 1) / kStepUnits;
    w.tiles = static_cast<int>((w.row_end - w.row_begin + kTileRows - 1) / kTileRows);

    for (int e = threadIdx.x; e < d; e += kThreads) qs[e] = to_f32(Q[static_cast<int64_t>(q) * d + e]);
    if (threadIdx.x == 0) {
        cnt = 0;
        thr = -INFINITY;
    }

    uint4 R[kStepUnits];
    on::load_step(R, w, 0, 0);
    // TAGS: the query's masks (block-uniform), and the position of this lane's row
    // one tile ahead, so that the gather of a tile's tags never waits for it
    uint64_t any_of = 0ull, none_of = 0ull;
    int32_t pos_next = -1;
    if constexpr (TAGS) {
        if (ta.any_of) any_of = ta.any_of[q];
        if (ta.none_of) none_of = ta.none_of[q];
        const int64_t row0 = w.row_begin + threadIdx.x;
        if (row0 < w.row_end) pos_next = row_pos[row0];
    }
    // the query's CSR row of every source: items xit[s][xlo[s], xhi[s]) (block-uniform)
    const int32_t* xit[on::kMaxSrc];
    int64_t xlo[on::kMaxSrc], xhi[on::kMaxSrc];
    if constexpr (LISTS) {
#pragma unroll
        for (int s = 0; s < on::kMaxSrc; ++s) {
            xit[s] = nullptr;
            xlo[s] = xhi[s] = 0;
            if (s < la.n) {
                const on::ListSrc& src = la.src[s];
                const int64_t r = src.rows ? src.rows[q] : static_cast<int64_t>(q);
                if (r >= 0 && r < src.n_rows) {
                    const int64_t lo = src.offsets[r], hi = src.offsets[r + 1];
                    xit[s] = src.items;
                    xlo[s] = lo;
                    xhi[s] = hi < lo ? lo : hi;
                }
            }
        }
        // while the first step is in flight: rows that fit the region together are
        // searched in LDS; the barrier below publishes them
        static_assert(on::kMaxSrc == 2, "ivf: the staging lays two sources side by side");
        const int64_t n0 = xhi[0] - xlo[0], n1 = xhi[1] - xlo[1];
        if (n0 <= kListCap && n1 <= kListCap - n0) {
            int32_t* const stg = reinterpret_cast<int32_t*>(lds + L::kBytes);
            for (int e = threadIdx.x; e < static_cast<int>(n0); e += kThreads) stg[e] = xit[0][xlo[0] + e];
            for (int e = threadIdx.x; e < static_cast<int>(n1); e += kThreads)
                stg[static_cast<int>(n0) + e] = xit[1][xlo[1] + e];
            xit[0] = xit[1] = stg;
            xlo[0] = 0;
            xhi[0] = xlo[1] = n0;
            xhi[1] = n0 + n1;
        }
    }
    __syncthreads();

    int over = 0;  // decided through the barrier that ends a tile: block-uniform (flatip_online_scan)
    for (int t = 0; t < w.tiles; ++t) {
        if (over) {
            if (wave == 0) {
                int n = cnt;
                float th = thr;
                compact_keep_ties(cand, n, k, on::kRoom, hist, th);
                if (lane == 0) {
                    cnt = n;
                    thr = th;
                }
            }
            __syncthreads();
        }
        const float th = thr;
        const int64_t row = w.row_begin + static_cast<int64_t>(t) * kTileRows + wave * 64 + lane;
        // original position of this lane's row: in flight under the scores
        int32_t pos;
        uint64_t tg = 0ull;
        if constexpr (TAGS) {
            pos = pos_next;
            // a position outside [0, n_pos) has no tags: no gather for it (it is dropped below)
            if (pos >= 0 && static_cast<int64_t>(pos) < n_pos) tg = ta.item_tags[pos];
            pos_next = (row + kTileRows) < w.row_end ? row_pos[row + kTileRows] : -1;
        } else {
            pos = row < w.row_end ? row_pos[row] : -1;
        }

        float acc[1];
        on::score_tile<T, 1>(R, w, t, stage, qs, d, acc);

        // ---- selection: at most one append per row ----
        // a position outside [0, n_pos) (a corrupt row_pos, an empty slot of a list with
        // slack) is dropped: it has no bit in the bitmap and no row in the caller's corpus
        bool pass = pos >= 0 && static_cast<int64_t>(pos) < n_pos && acc[0] >= th;
        if constexpr (TAGS) pass = pass && on::tag_eligible(tg, any_of, none_of);
        if constexpr (LISTS) {
            if (__any(pass)) {  // wave-uniform
#pragma unroll
                for (int s = 0; s < on::kMaxSrc; ++s) {
                    if (xhi[s] <= xlo[s]) continue;  // block-uniform
                    const bool listed = list_has(xit[s], xlo[s], xhi[s], pos, pass);  // every lane calls
                    pass = pass && !listed;
                }
            }
        } else if (excl && pass)
            pass = ((excl[static_cast<int64_t>(q) * excl_words + (pos >> 5)] >> (pos & 31)) & 1u) == 0u;
        over = __syncthreads_or(on::append<true>(pass, &cnt, cand, acc[0], static_cast<uint32_t>(pos)));
    }

    if (wave == 0) on::write_block_list(cand, cnt, k, hist, out, lists);
}

// ---- rt_segment_mean_f32 ----
// One block per segment. Thread (g, u) sums 16-byte unit u of the rows g, g + G,
// g + 2G, ... of the segment in fp64 (G = 256 / units row groups: consecutive
// threads read consecutive 16 bytes), then element e is the sum of its G
// partials in ascending g: the order depends on the segment's length and d
// only. No atomics.
constexpr int kMeanThreads = 256;

template <typename T>
__global__ __launch_bounds__(kMeanThreads) void segment_mean(const char* __restrict__ X, int64_t n, int d,
                                                             const int64_t* __restrict__ offsets,
                                                             const float* __restrict__ prev, int normalize,
                                                             float* __restrict__ out) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));
    __shared__ double part[kMeanThreads * EPU];  // [g][u][e]
    __shared__ double mean[256];
    const int64_t s = blockIdx.x;
    int64_t lo = offsets[s], hi = offsets[s + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    float* const o = out + s * d;
    if (hi <= lo) {  // block-uniform
        for (int e = threadIdx.x; e < d; e += kMeanThreads) o[e] = prev[s * d + e];
        return;
    }
    const int units = d / EPU;            // <= 64
    const int G = kMeanThreads / units;   // >= 4
    const int g = threadIdx.x / units, u = threadIdx.x - g * units;
    double acc[EPU];
#pragma unroll
    for (int e = 0; e < EPU; ++e) acc[e] = 0.0;
    if (g < G) {
        for (int64_t r = lo + g; r < hi; r += G) {
            const uint4 v = *reinterpret_cast<const uint4*>(X + (r * units + u) * 16);
            float x[EPU];
            on::widen(v, x, T());
#pragma unroll
            for (int e = 0; e < EPU; ++e) acc[e] += static_cast<double>(x[e]);
        }
#pragma unroll
        for (int e = 0; e < EPU; ++e) part[(g * units + u) * EPU + e] = acc[e];
    }
    __syncthreads();
    const double inv = 1.0 / static_cast<double>(hi - lo);
    for (int e = threadIdx.x; e < d; e += kMeanThreads) {
        double t = 0.0;
        for (int gg = 0; gg < G; ++gg) t += part[gg * d + e];  // (gg * units + e / EPU) * EPU + e % EPU
        mean[e] = t * inv;
    }
    __syncthreads();
    double scale = 1.0;
    if (normalize) {
        double ss = 0.0;
        for (int e = 0; e < d; ++e) ss += mean[e] * mean[e];  // LDS broadcast reads, the same order in every thread
        if (ss > 0.0) scale = 1.0 / sqrt(ss);
    }
    for (int e = threadIdx.x; e < d; e += kMeanThreads) o[e] = static_cast<float>(mean[e] * scale);
}

}  // namespace ivf
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace iv = rt::topk::ivf;
namespace ivon = rt::topk::online;

static_assert(RT_IVF_MAX_NPROBE == iv::kMaxProbe && RT_IVF_MAX_K == ivon::kMaxK, "rtrec_hip.h restates the kernel's limits");

static int g_ivf_min_tiles = 1;

extern "C" int rt_ivf_topk_tuning(int min_chunk_tiles) {
    if (min_chunk_tiles < 0 || min_chunk_tiles > 4096) return RT_ERR_INVALID;
    g_ivf_min_tiles = min_chunk_tiles ? min_chunk_tiles : 1;
    return RT_OK;
}

extern "C" int rt_ivf_topk_plan(int64_t nq, int nprobe, int64_t max_list_rows, int64_t* out) {
    if (nq <= 0 || nprobe <= 0 || max_list_rows < 0 || !out) return RT_ERR_INVALID;
    if (nprobe > iv::kMaxProbe || nq > iv::kMaxNq || max_list_rows >= 0xFFFFFFFFll) return RT_ERR_UNSUPPORTED;
    const iv::Plan p = iv::make_plan(nprobe, max_list_rows, g_ivf_min_tiles);
    out[0] = p.chunks;
    out[1] = p.rows_per_chunk;
    out[2] = nq * nprobe * p.chunks;
    return RT_OK;
}

extern "C" size_t rt_ivf_topk_workspace_bytes(int64_t nq, int nprobe, int64_t max_list_rows, int k) {
    int64_t plan[3];
    if (k <= 0 || k > ivon::kMaxK || rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK) return 256;
    const size_t need = static_cast<size_t>(plan[2]) * k * sizeof(uint64_t);
    return need < 256 ? 256 : need;
}

// the four entry points: the dense bitmap (la == nullptr) or the lists; list_len ==
// nullptr and n_pos == nx (rt_ivf_topk, rt_ivf_topk_lists) or the lists with slack
static int ivf_search(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                      const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                      const int32_t* row_pos, const int64_t* probes,
                      int nprobe, int64_t max_list_rows, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                      const ivon::ListArgs<true>* la, const ivon::TagSrc* tags, float* out_scores, int64_t* out_ids,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0 || n_pos < 0)
        return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !out_scores || !out_ids || !list_offsets || !probes || (nx > 0 && (!rows || !row_pos)))
        return RT_ERR_INVALID;
    if (k > ivon::kMaxK || nprobe > iv::kMaxProbe || nq > iv::kMaxNq) return RT_ERR_UNSUPPORTED;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!ivon::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll || n_pos >= 0x7FFFFFFFll || max_list_rows >= 0xFFFFFFFFll)
        return RT_ERR_UNSUPPORTED;  // positions are int32
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(rows)) & 15) return RT_ERR_INVALID;
    if (exclude_bits && exclude_words < (n_pos + 31) / 32) return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return RT_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const iv::Plan p = iv::make_plan(nprobe, max_list_rows, g_ivf_min_tiles);
    const int lists = nprobe * p.chunks;
    uint64_t* partials = static_cast<uint64_t*>(workspace);
    const dim3 grid(static_cast<unsigned>(lists), static_cast<unsigned>(nq)), block(ivon::kThreads);
    const char* x = static_cast<const char*>(rows);
#define RT_IVF_LAUNCH_T(T, LISTS, TAGS, LA, TA)                                                                  \
    hipLaunchKernelGGL((iv::ivf_scan<T, LISTS, TAGS>), grid, block, 0, st, static_cast<const T*>(queries), x, nx, \
                       d, k, list_offsets, nlist, list_len, n_pos, row_pos, probes, nprobe, p.chunks,             \
                       p.rows_per_chunk, exclude_bits, exclude_words, partials, LA, TA)
#define RT_IVF_LAUNCH(T, LISTS, LA) RT_IVF_LAUNCH_T(T, LISTS, false, LA, ivon::TagArgs<false>())
    if (tags) {  // with la, of any number of sources
        ivon::TagArgs<true> ta;
        static_cast<ivon::TagSrc&>(ta) = *tags;
        switch (dtype) {
            case RT_F32: RT_IVF_LAUNCH_T(float, true, true, *la, ta); break;
            case RT_F16: RT_IVF_LAUNCH_T(__half, true, true, *la, ta); break;
            default: RT_IVF_LAUNCH_T(__hip_bfloat16, true, true, *la, ta); break;
        }
    } else if (la) {
        switch (dtype) {
            case RT_F32: RT_IVF_LAUNCH(float, true, *la); break;
            case RT_F16: RT_IVF_LAUNCH(__half, true, *la); break;
            default: RT_IVF_LAUNCH(__hip_bfloat16, true, *la); break;
        }
    } else {
        const ivon::ListArgs<false> none{};
        switch (dtype) {
            case RT_F32: RT_IVF_LAUNCH(float, false, none); break;
            case RT_F16: RT_IVF_LAUNCH(__half, false, none); break;
            default: RT_IVF_LAUNCH(__hip_bfloat16, false, none); break;
        }
    }
#undef RT_IVF_LAUNCH
#undef RT_IVF_LAUNCH_T
    int rc = check_launch("ivf_scan");
    if (rc) return rc;
    return ivon::launch_finish(partials, lists, k, out_scores, out_ids, 0, nq, st);
}

extern "C" int rt_ivf_topk(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                           const int64_t* list_offsets, int64_t nlist, const int32_t* row_pos,
                           const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                           const uint32_t* exclude_bits, int64_t exclude_words, float* out_scores,
                           int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    return ivf_search(queries, nq, rows, nx, d, dtype, list_offsets, nlist, nullptr, nx, row_pos, probes, nprobe,
                      max_list_rows, k, exclude_bits, exclude_words, nullptr, nullptr, out_scores, out_ids, workspace,
                      workspace_bytes, stream);
}

extern "C" int rt_ivf_topk_lens(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                                const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows,
                                int k, const uint32_t* exclude_bits, int64_t exclude_words, float* out_scores,
                                int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    if (!list_len && nq > 0) return RT_ERR_INVALID;
    return ivf_search(queries, nq, rows, nx, d, dtype, list_offsets, nlist, list_len, n_pos, row_pos, probes, nprobe,
                      max_list_rows, k, exclude_bits, exclude_words, nullptr, nullptr, out_scores, out_ids, workspace,
                      workspace_bytes, stream);
}

static int ivf_search_lists(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                            const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                            const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                            const RtExclusionLists* lists, int n_lists, const RtTagFilter* filter,
                            float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                            void* stream) {
    ivon::TagSrc tags{};
    if (filter) {
        if (!filter->item_tags && n_pos > 0) return RT_ERR_INVALID;
        if ((reinterpret_cast<uintptr_t>(filter->item_tags) | reinterpret_cast<uintptr_t>(filter->any_of) |
             reinterpret_cast<uintptr_t>(filter->none_of)) & 7)
            return RT_ERR_INVALID;
        tags = ivon::TagSrc{filter->item_tags, filter->any_of, filter->none_of};
    }
    if (n_lists < 0 || (n_lists > 0 && !lists)) return RT_ERR_INVALID;
    if (n_lists > RT_ONLINE_MAX_EXCL_SOURCES) return RT_ERR_UNSUPPORTED;
    ivon::ListArgs<true> la{};
    la.n = n_lists;
    for (int s = 0; s < n_lists; ++s) {
        const RtExclusionLists& L = lists[s];
        if (!L.offsets || L.n_rows < 0 || (L.n_rows > 0 && !L.items)) return RT_ERR_INVALID;
        la.src[s] = ivon::ListSrc{L.offsets, L.items, L.rows, L.n_rows};
    }
    // no source and no filter: the plain scan, bit for bit rt_ivf_topk without a bitmap
    return ivf_search(queries, nq, rows, nx, d, dtype, list_offsets, nlist, list_len, n_pos, row_pos, probes, nprobe,
                      max_list_rows, k, nullptr, 0, (n_lists || filter) ? &la : nullptr, filter ? &tags : nullptr,
                      out_scores, out_ids, workspace, workspace_bytes, stream);
}

extern "C" int rt_ivf_topk_lists(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                 const int64_t* list_offsets, int64_t nlist, const int32_t* row_pos,
                                 const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                                 const RtExclusionLists* lists, int n_lists, float* out_scores, int64_t* out_ids,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return ivf_search_lists(queries, nq, rows, nx, d, dtype, list_offsets, nlist, nullptr, nx, row_pos, probes, nprobe,
                            max_list_rows, k, lists, n_lists, nullptr, out_scores, out_ids, workspace, workspace_bytes,
                            stream);
}

extern "C" int rt_ivf_topk_lists_lens(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                      const int64_t* list_offsets, int64_t nlist, const int64_t* list_len,
                                      int64_t n_pos, const int32_t* row_pos, const int64_t* probes, int nprobe,
                                      int64_t max_list_rows, int k, const RtExclusionLists* lists, int n_lists,
                                      float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    if (!list_len && nq > 0) return RT_ERR_INVALID;
    return ivf_search_lists(queries, nq, rows, nx, d, dtype, list_offsets, nlist, list_len, n_pos, row_pos, probes,
                            nprobe, max_list_rows, k, lists, n_lists, nullptr, out_scores, out_ids, workspace,
                            workspace_bytes, stream);
}

extern "C" int rt_ivf_topk_tags(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                                const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows,
                                int k, const RtExclusionLists* lists, int n_lists, const RtTagFilter* filter,
                                float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                                void* stream) {
    // list_len == NULL: lists without slack, positions are valid in [0, nx)
    return ivf_search_lists(queries, nq, rows, nx, d, dtype, list_offsets, nlist, list_len, list_len ? n_pos : nx,
                            row_pos, probes, nprobe, max_list_rows, k, lists, n_lists, filter, out_scores, out_ids,
                            workspace, workspace_bytes, stream);
}

extern "C" int rt_segment_mean_f32(const void* rows, int64_t n, int d, int dtype, const int64_t* offsets,
                                   int64_t n_seg, const float* prev, int normalize, float* out, void* stream) {
    if (n < 0 || d <= 0 || n_seg < 0) return RT_ERR_INVALID;
    if (n_seg == 0) return RT_OK;
    if (!offsets || !prev || !out || (n > 0 && !rows)) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!ivon::shape_ok(d, dtype) || n_seg > 0x7FFFFFFFll) return RT_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(rows) & 15) return RT_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const dim3 grid(static_cast<unsigned>(n_seg)), block(iv::kMeanThreads);
    const char* x = static_cast<const char*>(rows);
    switch (dtype) {
        case RT_F32:
            hipLaunchKernelGGL((iv::segment_mean<float>), grid, block, 0, st, x, n, d, offsets, prev, normalize, out);
            break;
        case RT_F16:
            hipLaunchKernelGGL((iv::segment_mean<__half>), grid, block, 0, st, x, n, d, offsets, prev, normalize, out);
            break;
        default:
            hipLaunchKernelGGL((iv::segment_mean<__hip_bfloat16>), grid, block, 0, st, x, n, d, offsets, prev,
                               normalize, out);
            break;
    }
    return check_launch("segment_mean");
}
