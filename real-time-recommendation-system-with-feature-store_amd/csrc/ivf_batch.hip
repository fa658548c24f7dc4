// IVF-Flat, list-major batch search (rt_ivf_topk_batch): one pass over a list
// for all queries of a tile that probe it. Serves faiss.IndexIVFFlat.search
// with a batch of users (src/serving/retrieval.py:141-197) and the offline
// evaluation. The per-query scan (ivf.hip) launches one block per (query,
// probed list, chunk) and streams the list again for each; here the work items
// are (list, tile of kQT queries that probe it, row chunk) and the scores of a
// tile come from the fp32 MFMA.
//
// Six launches, all sized by host arguments (no host read, stream-ordered,
// capturable):
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
#include "ivf_batch_plan.h"
#include "topk_online.h"

namespace rt {
namespace topk {
namespace ivfb {

namespace on = rt::topk::online;

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kKC = 32;             // d per LDS chunk
constexpr int kLS = kKC + 4;        // row stride (floats): 144 B, conflict-free b128 fragment reads
constexpr int kQS = 256 + 4;        // query stride (floats): the same bank pattern
constexpr int kCap = 320;           // candidate buffer of one query
constexpr int kRoom = kCap - kTileRows;
static_assert(kTileRows == 32 * kWaves, "ivf batch: a wave scores one 32-row MFMA tile per step");
static_assert(kRoom >= kMaxK, "ivf batch: a compaction must be able to keep the k best");
static_assert(kMaxK <= v4::kFinishCap, "ivf batch: the block's list is sorted by the 128-entry register sort");
static_assert(kMaxLists == on::kMaxBlocks && kMaxK == on::kMaxK, "ivf_batch_plan.h restates the finish's limits");

struct Lds {
    static constexpr int kRows = 2 * kTileRows * kLS * 4;
    static constexpr int kQuery = kQT * kQS * 4;
    static constexpr int kCand = kQT * kCap * static_cast<int>(sizeof(Cand));
    static constexpr int kHist = kWaves * 256 * 4;
    static constexpr int kBytes = kRows + kQuery + kCand + kHist;
    // one block per CU; 1 KiB left for the block's small arrays and the barrier's reduction
    static_assert(kBytes + 1024 <= 163840, "ivf batch: the block's LDS");
};

// zero `bytes` (a multiple of 4) from an 8-byte aligned base: the partial lists and the counts
__global__ __launch_bounds__(256) void ivfb_zero(uint64_t* __restrict__ base, size_t bytes) {
    const size_t n8 = bytes / 8;
    const size_t step = static_cast<size_t>(gridDim.x) * 256;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n8; i += step) base[i] = 0ull;
    if ((bytes & 4) && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<uint32_t*>(base)[2 * n8] = 0u;
}

__global__ __launch_bounds__(256) void ivfb_count(const int64_t* __restrict__ probes, int64_t pairs, int64_t nlist,
                                                  int32_t* __restrict__ count, int32_t* __restrict__ rank) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int64_t l = probes[p];
    rank[p] = (l >= 0 && l < nlist) ? atomicAdd(&count[l], 1) : -1;
}

// one block: thread t owns the lists [t seg, (t + 1) seg)
__global__ __launch_bounds__(1024) void ivfb_offsets(const int32_t* __restrict__ count, int64_t nlist,
                                                     int32_t* __restrict__ pair_start,
                                                     int32_t* __restrict__ tile_start) {
    __shared__ int sp[1024], st[1024];
    const int t = threadIdx.x;
    const int64_t seg = (nlist + 1023) / 1024;
    const int64_t a = t * seg < nlist ? t * seg : nlist, b = (a + seg) < nlist ? (a + seg) : nlist;
    int np = 0, nt = 0;
    for (int64_t l = a; l < b; ++l) {
        const int c = count[l];
        np += c;
        nt += (c + kQT - 1) / kQT;
    }
    sp[t] = np;
    st[t] = nt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int up = t >= o ? sp[t - o] : 0, ut = t >= o ? st[t - o] : 0;
        __syncthreads();
        sp[t] += up;
        st[t] += ut;
        __syncthreads();
    }
    int bp = sp[t] - np, bt = st[t] - nt;
    for (int64_t l = a; l < b; ++l) {
        const int c = count[l];
        pair_start[l] = bp;
        tile_start[l] = bt;
        bp += c;
        bt += (c + kQT - 1) / kQT;
    }
    if (t == 1023) {
        pair_start[nlist] = sp[t];
        tile_start[nlist] = st[t];
    }
}

__global__ __launch_bounds__(256) void ivfb_scatter(const int64_t* __restrict__ probes, int64_t pairs, int64_t nlist,
                                                    const int32_t* __restrict__ pair_start,
                                                    const int32_t* __restrict__ rank, int32_t* __restrict__ out) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int64_t l = probes[p];
    const int r = rank[p];
    // probes may change between two launches of a call only by the caller's error: the
    // slot is tested all the same, so that nothing is written outside `out`
    if (l >= 0 && l < nlist && r >= 0) {
        const int64_t at = static_cast<int64_t>(pair_start[l]) + r;
        if (at < pairs) out[at] = static_cast<int32_t>(p);
    }
}

// wave: compact one candidate buffer; thr = the lowest score kept (ivf.hip)
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
    const int T_ = static_cast<int>(blockIdx.x / static_cast<unsigned>(chunks));
    const int c = static_cast<int>(blockIdx.x - static_cast<unsigned>(T_) * static_cast<unsigned>(chunks));
    if (T_ >= tile_start[nlist]) return;  // block-uniform: a surplus block of the host bound
    int64_t l;
    {
        int64_t lo = 0, hi = nlist - 1;  // the first list with tile_start[l + 1] > T_ (one exists)
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (tile_start[mid + 1] > T_) hi = mid;
            else lo = mid + 1;
        }
        l = lo;
    }
    // The tables are this call's own (ivfb_offsets), and consistent ones give 0 <= p0 < p1 <=
    // n_pairs; the block tests it all the same (in 64 bits), and every pair id below, so that no
    // table contents can take a read outside `pairs` or a write outside the partial lists.
    const int64_t p0 = pair_start[l] + (static_cast<int64_t>(T_) - tile_start[l]) * kQT;
    int64_t p1 = pair_start[l + 1];
    p1 = p1 < n_pairs ? p1 : n_pairs;
    if (p0 < 0 || p0 >= p1) return;  // block-uniform
    const int nqt = (p1 - p0) < kQT ? static_cast<int>(p1 - p0) : kQT;

    // the chunk, clamped to the list and to the corpus (ivf_scan's window)
    int64_t row_begin = 0, row_end = 0;
    {
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
                row_begin = lo + first;
                row_end = (first + rows_per_chunk) < len ? (row_begin + rows_per_chunk) : hi;
            }
        }
    }
    if (row_end <= row_begin) return;  // block-uniform: the partial lists were zeroed

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
    if (tid < kQT) {
        int pid = -1;
        if (tid < nqt) pid = pairs[p0 + tid];
        const bool ok = pid >= 0 && pid < n_pairs;
        const int q = ok ? pid / nprobe : -1;  // -1: no query in this slot of the tile
        qid[tid] = q;
        qslot[tid] = ok ? pid - q * nprobe : 0;
        cnt[tid] = 0;
        thr[tid] = -INFINITY;
    }
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
            int mine_over = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = tile_row(r, half);
                bool pass = valid && qid[qi] >= 0 && acc[r] >= thr[qi];
                if (excl && pass)
                    pass = ((excl[static_cast<int64_t>(qid[qi]) * excl_words + (pos >> 5)] >> (pos & 31)) & 1u) == 0u;
                const uint64_t bm = __ballot(pass);
                if (bm) {  // wave-uniform
                    // one LDS atomic per lane half: the halves hold different queries
                    const uint32_t mine = half ? static_cast<uint32_t>(bm >> 32) : static_cast<uint32_t>(bm);
                    const int n_mine = __popc(mine);
                    int base = 0;
                    if (col == 0 && n_mine) base = atomicAdd(&cnt[qi], n_mine);
                    base = __shfl(base, half * 32, 64);
                    const int at = base + __popc(mine & ((1u << col) - 1u));
                    // guarded: a row_pos that repeats positions gives equal keys, of which a
                    // compaction may keep more than its limit
                    if (pass && at < kCap) cand[qi * kCap + at] = Cand{acc[r], static_cast<uint32_t>(pos)};
                    mine_over |= (base + n_mine) > kRoom ? 1 : 0;
                }
            }
            acc = f32x16{};
            over = __syncthreads_or(mine_over);
            if (over && more) {
                for (int qi = wave; qi < nqt; qi += kWaves) {
                    int n = cnt[qi] < kCap ? cnt[qi] : kCap;
                    if (n > kRoom) {
                        float th = thr[qi];
                        // down to the finish's 128, not to kRoom: a buffer left near kRoom
                        // passes the check again after the next tile's first appends
                        compact_keep_ties(cand + qi * kCap, n, k, v4::kFinishCap, hist, th);
                        if (lane == 0) {
                            cnt[qi] = n;
                            thr[qi] = th;
                        }
                    }
                }
                __syncthreads();
            }
        }
        rt = nrt;
        cc = ncc;
    }

    // ---- the block's list per query: partials[query][rank][slot x chunks + c] ----
    const int lists = nprobe * chunks;
    for (int qi = wave; qi < nqt; qi += kWaves) {
        if (qid[qi] < 0) continue;  // wave-uniform
        const int n = cnt[qi] < kCap ? cnt[qi] : kCap;
        on::write_block_list(cand + qi * kCap, n, k, hist,
                             partials + static_cast<int64_t>(qid[qi]) * k * lists + qslot[qi] * chunks + c, lists);
    }
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
    const size_t pbytes = ib::partial_bytes(nq, nprobe, k, p);
    uint64_t* const partials = static_cast<uint64_t*>(workspace);
    int32_t* const count = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + pbytes);
    int32_t* const pair_start = count + nlist;
    int32_t* const tile_start = pair_start + nlist + 1;
    int32_t* const rank = tile_start + nlist + 1;
    int32_t* const pair_of = rank + pairs;
    const int stages = g_ivfb_stages;
    int rc = RT_OK;
    if (stages & 1) {
        // the partial lists and the counts lie side by side: one fill launch
        const size_t zbytes = pbytes + static_cast<size_t>(nlist) * 4;
        const size_t zblocks = (zbytes / 8 + 2047) / 2048;  // 8 words per thread, at most
        hipLaunchKernelGGL(ib::ivfb_zero, dim3(static_cast<unsigned>(zblocks < 1 ? 1 : (zblocks > 4096 ? 4096 : zblocks))),
                           dim3(256), 0, st, partials, zbytes);
        rc = check_launch("ivfb_zero");
        if (rc) return rc;
        const unsigned pblocks = static_cast<unsigned>((pairs + 255) / 256);
        hipLaunchKernelGGL(ib::ivfb_count, dim3(pblocks), dim3(256), 0, st, probes, pairs, nlist, count, rank);
        rc = check_launch("ivfb_count");
        if (rc) return rc;
        hipLaunchKernelGGL(ib::ivfb_offsets, dim3(1), dim3(1024), 0, st, count, nlist, pair_start, tile_start);
        rc = check_launch("ivfb_offsets");
        if (rc) return rc;
        hipLaunchKernelGGL(ib::ivfb_scatter, dim3(pblocks), dim3(256), 0, st, probes, pairs, nlist, pair_start, rank,
                           pair_of);
        rc = check_launch("ivfb_scatter");
        if (rc) return rc;
    }
    if (!(stages & 6)) return RT_OK;
    if (!(stages & 2)) return ibon::launch_finish(partials, nprobe * p.chunks, k, out_scores, out_ids, 0, nq, st);
    const dim3 grid(static_cast<unsigned>(p.blocks)), block(ib::kThreads);
    const char* x = static_cast<const char*>(rows);
#define RT_IVFB_LAUNCH(T)                                                                                          \
    hipLaunchKernelGGL((ib::ivfb_scan<T>), grid, block, 0, st, static_cast<const T*>(queries), x, nx, d, k,        \
                       list_offsets, nlist, list_len, n_pos, row_pos, nprobe, p.chunks, p.rows_per_chunk,          \
                       exclude_bits, exclude_words, partials, pair_start, tile_start, pair_of,                     \
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
