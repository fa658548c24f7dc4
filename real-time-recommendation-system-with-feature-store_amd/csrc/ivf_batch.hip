// IVF-Flat, list-major batch search (rt_ivf_topk_batch): one pass over a list
// for all queries of a tile that probe it. Serves faiss.IndexIVFFlat.search
// with a batch of users (src/serving/retrieval.py:141-197) and the offline
// evaluation. The per-query scan (ivf.hip) launches one block per (query,
// probed list, chunk) and streams the list again for each; here the work items
// are (list, tile of kQT queries that probe it, row chunk) and the scores of a
// tile come from the fp32 MFMA.
//
// Six launches, all sized by host arguments (no host read, stream-ordered,
// capturable). Launches 0-3, the work item of a scan block and everything
// behind the score live in ivf_batch_group.h, shared with ivf_sq8_batch.hip:
//
// 0. ivfb_zero: the partial lists and the per-list counts are zeroed: a partial
//    list that no work item writes (a skipped probe, a chunk past its list)
//    reads "none". A launch of the call's own, not a memset: a captured call
//    is then a chain of kernel nodes only.
// 1. ivfb_count: one thread per (query, probe slot) pair p = q x nprobe + slot;
//    a valid list id takes rank[p] = atomicAdd(count[list], 1).
// 2. ivfb_offsets: one block; exclusive prefix sums over the lists of the pair
//    counts (pair_start) and of ceil(count / kQT) (tile_start).
// 3. ivfb_scatter: pairs[pair_start[list] + rank[p]] = p. The order of the pairs
//    of a list depends on the atomics; it does not reach the result, because
//    every pair owns its own partial lists.
// 4. ivfb_scan: block b = (tile number T = b / chunks, chunk c = b % chunks);
//    T >= tile_start[nlist] leaves (the grid is the host bound of the plan). A
//    bisection of tile_start gives the list; the block stages the tile's
//    queries once as fp32 (gathered through `pairs`), clamps chunk c of the
//    list exactly as ivf_scan does, and streams the rows through LDS in 32-wide
//    column chunks (register-prefetched one chunk ahead, double-buffered), each
//    row as [even d | odd d] of the chunk so that one ds_read_b128 feeds four
//    k-steps — the layout of dense_scores_kernel (topk_dense.h). Wave w scores
//    rows 32 w .. 32 w + 31 of the 128-row tile against the 32 queries with
//    v_mfma_f32_32x32x2_f32: every score is one accumulation chain over d in
//    increasing order, the sequential fmaf chain of oracle/flatip.c; 16-bit
//    rows and queries are widened to fp32 first (every product is exact), as
//    in the per-query scan. Only k-steps inside d are issued: a padded step
//    would turn a -0.0 sum into +0.0.
//    Selection: the lane of row `col` holds 16 scores, of queries tile_row(r,
//    half); a score at or above its query's threshold (and whose position
//    passes the range and bitmap tests) is appended to the query's LDS
//    candidate buffer, one LDS atomic per lane half. A buffer above kRoom is
//    compacted before the next tile (v4::compact_stream, the decision taken
//    through the barrier that ends the tile); the threshold after a compaction
//    is the lowest score kept, because rows do not arrive in position order.
//    At the end every query's list goes out sorted, as composite keys, to
//    partials[query][rank][slot x chunks + c] — the format of the per-query
//    scan.
// 5. flatip_online_finish (topk_online.h, unchanged), one block per query over
//    its nprobe x chunks <= 512 partial lists.
#include "ivf_batch_group.h"

namespace rt {
namespace topk {
namespace ivfb {

constexpr int kKC = 32;             // d per LDS chunk
constexpr int kLS = kKC + 4;        // row stride (floats): 144 B, conflict-free b128 fragment reads
constexpr int kQS = 256 + 4;        // query stride (floats): the same bank pattern

struct Lds {
    static constexpr int kRows = 2 * kTileRows * kLS * 4;
    static constexpr int kQuery = kQT * kQS * 4;
    static constexpr int kCand = kQT * kCap * static_cast<int>(sizeof(Cand));
    static constexpr int kHist = kWaves * 256 * 4;
    static constexpr int kBytes = kRows + kQuery + kCand + kHist;
    // one block per CU; 1 KiB left for the block's small arrays and the barrier's reduction
    static_assert(kBytes + 1024 <= 163840, "ivf batch: the block's LDS");
};

template <typename T>
__global__ __launch_bounds__(kThreads, 1) void ivfb_scan(
    const T* __restrict__ Q, const char* __restrict__ X, int64_t nx, int d, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int64_t* __restrict__ list_len, int64_t n_pos,
    const int32_t* __restrict__ row_pos, int nprobe, int chunks, int64_t rows_per_chunk,
    const uint32_t* __restrict__ excl, int64_t excl_words, uint64_t* __restrict__ partials,
    const int32_t* __restrict__ pair_start, const int32_t* __restrict__ tile_start,
    const int32_t* __restrict__ pairs, int n_pairs) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));  // elements per 16-byte unit
    constexpr int UPR = kKC / EPU;                         // units of a row per column chunk
    constexpr int NU = kTileRows * UPR / kThreads;         // units a thread moves per step
    __shared__ __attribute__((aligned(16))) char lds[Lds::kBytes];
    __shared__ int cnt[kQT];
    __shared__ float thr[kQT];
    __shared__ int qid[kQT], qslot[kQT];
    float* const rows_l = reinterpret_cast<float*>(lds);
    float* const qs = reinterpret_cast<float*>(lds + Lds::kRows);
    Cand* const cand = reinterpret_cast<Cand*>(lds + Lds::kRows + Lds::kQuery);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + Lds::kRows + Lds::kQuery + Lds::kCand) + wave * 256;

    // ---- the work item: (list, query tile, chunk) ----
    Item w;
    if (!work_item(pair_start, tile_start, n_pairs, chunks, list_offsets, nlist, list_len, nx, rows_per_chunk, w))
        return;  // block-uniform
    const int nqt = w.nqt;
    const int64_t row_begin = w.row_begin, row_end = w.row_end;

    const int64_t row_bytes = static_cast<int64_t>(d) * static_cast<int64_t>(sizeof(T));
    const int nchunks = (d + kKC - 1) / kKC;
    const int tiles = static_cast<int>((row_end - row_begin + kTileRows - 1) / kTileRows);
    const int total = tiles * nchunks;

    uint4 R[NU];
    // step (tile rt, column chunk cc): unit f = i * 256 + tid is unit f % UPR of tile row f / UPR
    auto load = [&](int rt, int cc) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int f = i * kThreads + tid;
            const int r = f / UPR, u = f - r * UPR;
            const int64_t row = row_begin + static_cast<int64_t>(rt) * kTileRows + r;
            const int e0 = cc * kKC + u * EPU;
            R[i] = make_uint4(0u, 0u, 0u, 0u);
            if (row < row_end && e0 < d)
                R[i] = *reinterpret_cast<const uint4*>(X + row * row_bytes + static_cast<int64_t>(e0) * sizeof(T));
        }
    };
    // [even d | odd d] within the chunk: element 2 s + h of the chunk lands at 16 h + s
    auto store = [&](int b) {
        float* const base = rows_l + b * (kTileRows * kLS);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int f = i * kThreads + tid;
            const int r = f / UPR, u = f - r * UPR;
            float x[EPU];
            on::widen(R[i], x, T());
            float* const row = base + r * kLS + u * (EPU / 2);
            if constexpr (EPU == 4) {
                *reinterpret_cast<float2*>(row) = make_float2(x[0], x[2]);
                *reinterpret_cast<float2*>(row + kKC / 2) = make_float2(x[1], x[3]);
            } else {
                *reinterpret_cast<float4*>(row) = make_float4(x[0], x[2], x[4], x[6]);
                *reinterpret_cast<float4*>(row + kKC / 2) = make_float4(x[1], x[3], x[5], x[7]);
            }
        }
    };

    load(0, 0);
    tile_slots(w, pairs, n_pairs, nprobe, qid, qslot, cnt, thr);
    __syncthreads();
    // the tile's queries as fp32, in the rows' chunk layout; padding queries and columns: zeros
    {
        const int dp = nchunks * kKC;
        for (int idx = tid; idx < kQT * dp; idx += kThreads) {
            const int i = idx / dp, e = idx - i * dp;
            float v = 0.f;
            if (qid[i] >= 0 && e < d) v = to_f32(Q[static_cast<int64_t>(qid[i]) * d + e]);
            const int w = e & (kKC - 1);
            qs[i * kQS + (e - w) + (w & 1) * (kKC / 2) + (w >> 1)] = v;
        }
    }
    store(0);
    __syncthreads();

    f32x16 acc = f32x16{};
    int32_t pos = -1;
    int over = 0;  // decided through the barrier that ends a tile: block-uniform
    int rt = 0, cc = 0;
    for (int stp = 0; stp < total; ++stp) {
        const int b = stp & 1;
        int nrt = rt, ncc = cc + 1;
        if (ncc == nchunks) {
            ncc = 0;
            nrt = rt + 1;
        }
        const bool more = stp + 1 < total;
        if (more) load(nrt, ncc);
        const int64_t row = row_begin + static_cast<int64_t>(rt) * kTileRows + wave * 32 + col;
        // original position of this lane's row: in flight under the scores
        if (cc == 0) pos = row < row_end ? row_pos[row] : -1;
        {
            const float* qa = qs + col * kQS + cc * kKC + half * (kKC / 2);
            const float* xa = rows_l + b * (kTileRows * kLS) + (wave * 32 + col) * kLS + half * (kKC / 2);
            // k-steps of this chunk inside d: 16, or fewer (an even number) in the last chunk
            const int steps = ((d - cc * kKC) < kKC ? (d - cc * kKC) : kKC) / 2;
#pragma unroll
            for (int s = 0; s < kKC / 2; s += 4) {
                if (s < steps) {  // wave-uniform
                    const float4 a = *reinterpret_cast<const float4*>(qa + s);
                    const float4 u = *reinterpret_cast<const float4*>(xa + s);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, u.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, u.y, acc, 0, 0, 0);
                    if (s + 2 < steps) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, u.z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, u.w, acc, 0, 0, 0);
                    }
                }
            }
        }
        if (more) store(b ^ 1);
        if (cc + 1 < nchunks) {
            __syncthreads();
        } else {
            // ---- selection: acc[r] = (query tile_row(r, half), row `col` of this wave) ----
            // a position outside [0, n_pos) (a corrupt row_pos, an empty slot of a list with
            // slack) is dropped: it has no bit in the bitmap and no row in the caller's corpus
            const bool valid = row < row_end && pos >= 0 && static_cast<int64_t>(pos) < n_pos;
            const int mine_over = select_tile(acc, valid, pos, qid, thr, cnt, cand, excl, excl_words);
            acc = f32x16{};
            over = __syncthreads_or(mine_over);
            if (over && more) {
                compact_tile_buffers(nqt, k, cnt, thr, cand, hist);
                __syncthreads();
            }
        }
        rt = nrt;
        cc = ncc;
    }

    write_tile_lists(w, k, nprobe, chunks, qid, qslot, cnt, cand, hist, partials);
}

}  // namespace ivfb
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace ib = rt::topk::ivfb;
namespace ibon = rt::topk::online;

static_assert(RT_IVF_MAX_NPROBE == ib::kMaxProbe && RT_IVF_MAX_K == ib::kMaxK, "rtrec_hip.h restates the kernel's limits");

// measurements only: which of {grouping, scan, finish} a call issues (0 = all)
static int g_ivfb_stages = 7;
int rt::topk::ivfb::stages() { return g_ivfb_stages; }

extern "C" int rt_ivf_topk_batch_tuning(int stages) {
    if (stages < 0 || stages > 7) return RT_ERR_INVALID;
    g_ivfb_stages = stages ? stages : 7;
    return RT_OK;
}

extern "C" int rt_ivf_topk_batch_plan(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows, int k,
                                      int64_t* out) {
    if (nq <= 0 || nprobe <= 0 || nlist <= 0 || max_list_rows < 0 || k <= 0 || !out) return RT_ERR_INVALID;
    ib::Plan p;
    if (!ib::make_plan(nq, nprobe, nlist, max_list_rows, k, p)) return RT_ERR_UNSUPPORTED;
    out[0] = p.qt;
    out[1] = p.rows_per_chunk;
    out[2] = p.chunks;
    out[3] = p.items_bound;
    out[4] = p.blocks;
    return RT_OK;
}

extern "C" size_t rt_ivf_topk_batch_workspace_bytes(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows,
                                                    int k) {
    ib::Plan p;
    if (!ib::make_plan(nq, nprobe, nlist, max_list_rows, k, p)) return 256;
    return ib::workspace_bytes(nq, nprobe, nlist, k, p);
}

extern "C" int rt_ivf_topk_batch(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                 const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                                 const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows,
                                 int k, const uint32_t* exclude_bits, int64_t exclude_words, float* out_scores,
                                 int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    if (!list_len) n_pos = nx;  // lists without slack: positions are valid in [0, nx)
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0 || n_pos < 0)
        return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !out_scores || !out_ids || !list_offsets || !probes || (nx > 0 && (!rows || !row_pos)))
        return RT_ERR_INVALID;
    if (k > ib::kMaxK || nprobe > ib::kMaxProbe) return RT_ERR_UNSUPPORTED;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!ibon::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll || n_pos >= 0x7FFFFFFFll) return RT_ERR_UNSUPPORTED;  // positions are int32
    ib::Plan p;
    if (!ib::make_plan(nq, nprobe, nlist, max_list_rows, k, p)) return RT_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(rows)) & 15) return RT_ERR_INVALID;
    if (exclude_bits && exclude_words < (n_pos + 31) / 32) return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < ib::workspace_bytes(nq, nprobe, nlist, k, p)) return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return RT_ERR_INVALID;

    hipStream_t st = as_stream(stream);
    const int64_t pairs = nq * nprobe;
    const ib::Tables t = ib::carve(workspace, nq, nprobe, nlist, k, p);
    uint64_t* const partials = t.partials;
    const int stages = g_ivfb_stages;
    int rc = RT_OK;
    if (stages & 1) {
        rc = ib::launch_grouping(t, probes, pairs, nlist, st);
        if (rc) return rc;
    }
    if (!(stages & 6)) return RT_OK;
    if (!(stages & 2)) return ibon::launch_finish(partials, nprobe * p.chunks, k, out_scores, out_ids, 0, nq, st);
    const dim3 grid(static_cast<unsigned>(p.blocks)), block(ib::kThreads);
    const char* x = static_cast<const char*>(rows);
#define RT_IVFB_LAUNCH(T)                                                                                          \
    hipLaunchKernelGGL((ib::ivfb_scan<T>), grid, block, 0, st, static_cast<const T*>(queries), x, nx, d, k,        \
                       list_offsets, nlist, list_len, n_pos, row_pos, nprobe, p.chunks, p.rows_per_chunk,          \
                       exclude_bits, exclude_words, partials, t.pair_start, t.tile_start, t.pair_of,               \
                       static_cast<int>(pairs))
    switch (dtype) {
        case RT_F32: RT_IVFB_LAUNCH(float); break;
        case RT_F16: RT_IVFB_LAUNCH(__half); break;
        default: RT_IVFB_LAUNCH(__hip_bfloat16); break;
    }
#undef RT_IVFB_LAUNCH
    rc = check_launch("ivfb_scan");
    if (rc || !(stages & 4)) return rc;
    return ibon::launch_finish(partials, nprobe * p.chunks, k, out_scores, out_ids, 0, nq, st);
}
