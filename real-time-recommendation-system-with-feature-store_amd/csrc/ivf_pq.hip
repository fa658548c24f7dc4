// IVF-PQ: product-quantised lists (faiss.index_factory(d, "IVF1024,PQ16"), the
// one-line config change of src/serving/retrieval.py:96-110). A row is M bytes:
// code[m] names one of 256 codewords of subspace m (dsub = d / M elements).
//
// rt_pq_encode, one launch: grid (row tiles, M). A block copies its subspace's
// 256 x dsub codebook into LDS (<= 32 KB), a lane keeps the sub-vectors of
// kEncRows rows in registers (the residual x - centroid[assign] when the call
// has centroids) and walks the 256 codewords in order: every lane reads the
// same LDS address (a broadcast, no bank conflicts), and the kEncRows
// independent chains per lane hide the LDS latency. The distance is the
// sequential chain acc = fmaf(r_j - c_j, r_j - c_j, acc), j ascending from 0;
// the lowest codeword wins ties (a strict <). No matrix instructions: they
// would need the |x|^2 - 2 x.c + |c|^2 form, which rounds differently and
// breaks the tie rule on equidistant codewords.
//
// rt_ivf_pq_topk, three launches (no host read, stream-ordered, capturable):
//
// 1. pq_tables: grid (query, M / 4). lut[q][m][c] = sum_j Q[q][m dsub + j]
//    cb[m][c][j], the fmaf chain from 0; thread c of the block reads codeword c
//    (consecutive threads read consecutive dsub x 4 bytes: coalesced), the
//    query sub-vector sits in LDS (broadcast reads). With residual encoding
//    q.x ~ q.c_list + sum_m lut[m][code_m]: the tables depend on the query
//    only, and q.c_list is the coarse search's score, passed as `bias`.
// 2. ivf_pq_scan: rt_ivf_topk's grid, (probe x chunk, query), its window
//    (chunk_window) and everything behind the score (pos_passes, bitmap_clear,
//    online::append<true>, compact_keep_ties, online::write_block_list). A
//    block copies its query's M KB table into LDS and needs no row stage; a
//    lane owns one row of a 256-row tile, reads its M code bytes as 16-byte
//    (M % 16 == 0) or 4-byte words — a wave reads 64 M contiguous bytes — one
//    tile ahead of the lookups, with the row's position. The score is acc =
//    bias, then acc += lut[m][code_m], m ascending. The table is laid out
//    [m][256]: the 64 lookups of a wave at one m fall on random banks, which
//    is inherent to ADC; the M lookups of a lane are independent of the chain
//    and of each other, so they are all issued before the first add waits.
//    LDS is sized by the table class (M <= 16, 32, 64 -> 16, 32, 64 KB) so
//    that a small M keeps more blocks per CU than the two M = 64 leaves.
// 3. flatip_online_finish (topk_online.h, unchanged).
#include "ivf_select.h"

namespace rt {
namespace topk {
namespace ivfpq {

namespace on = rt::topk::online;
namespace iv = rt::topk::ivf;

constexpr int kMinM = 4, kMaxM = 64, kMaxDsub = 32, kCodewords = 256;

// ---- rt_pq_encode ----
constexpr int kEncThreads = 128;
constexpr int kEncRows = 2;  // rows per lane
constexpr int kEncTile = kEncThreads * kEncRows;
static_assert(kCodewords * kMaxDsub * 4 <= 32768, "pq_encode: a subspace's codebook takes <= 32 KB of LDS");

// two consecutive elements of a row, widened; e % 2 == 0 and rows 16-byte aligned
__device__ __forceinline__ float2 load2(const void* rows, int dtype, int64_t e) {
    if (dtype == RT_F32) return *reinterpret_cast<const float2*>(static_cast<const float*>(rows) + e);
    const uint32_t v = *reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(rows) + e);
    const uint16_t lo = static_cast<uint16_t>(v & 0xFFFFu), hi = static_cast<uint16_t>(v >> 16);
    if (dtype == RT_F16) return make_float2(bits_f16_to_f32(lo), bits_f16_to_f32(hi));
    return make_float2(bits_bf16_to_f32(lo), bits_bf16_to_f32(hi));
}

template <int DSUB>
__global__ __launch_bounds__(kEncThreads) void pq_encode(const void* __restrict__ rows, int64_t n, int d, int dtype,
                                                         const float* __restrict__ centroids, int64_t nlist,
                                                         const int64_t* __restrict__ assign,
                                                         const float* __restrict__ codebooks, int M,
                                                         uint8_t* __restrict__ codes) {
    __shared__ __attribute__((aligned(16))) float cb[kCodewords * DSUB];
    const int m = blockIdx.y;
    const float4* src = reinterpret_cast<const float4*>(codebooks + static_cast<int64_t>(m) * kCodewords * DSUB);
    for (int e = threadIdx.x; e < kCodewords * DSUB / 4; e += kEncThreads) reinterpret_cast<float4*>(cb)[e] = src[e];

    float r[kEncRows][DSUB];
    int64_t row[kEncRows];
#pragma unroll
    for (int i = 0; i < kEncRows; ++i) {
        row[i] = static_cast<int64_t>(blockIdx.x) * kEncTile + i * kEncThreads + threadIdx.x;
        const bool valid = row[i] < n;
        int64_t l = -1;
        if (valid && centroids) l = assign[row[i]];
        const bool resid = l >= 0 && l < nlist;
#pragma unroll
        for (int j = 0; j < DSUB; j += 2) {  // the compiler merges neighbouring pairs into wider loads
            float2 x = make_float2(0.f, 0.f);
            if (valid) x = load2(rows, dtype, row[i] * d + m * DSUB + j);
            if (resid) {
                const float2 c = *reinterpret_cast<const float2*>(centroids + l * d + m * DSUB + j);
                x.x = x.x - c.x;
                x.y = x.y - c.y;
            }
            r[i][j] = x.x;
            r[i][j + 1] = x.y;
        }
    }
    __syncthreads();

    float best[kEncRows];
    int code[kEncRows];
#pragma unroll
    for (int i = 0; i < kEncRows; ++i) {
        best[i] = INFINITY;
        code[i] = 0;
    }
    for (int c = 0; c < kCodewords; ++c) {
        float acc[kEncRows];
#pragma unroll
        for (int i = 0; i < kEncRows; ++i) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < DSUB; j += 2) {
            const float2 w = *reinterpret_cast<const float2*>(cb + c * DSUB + j);  // wave-uniform: a broadcast
#pragma unroll
            for (int i = 0; i < kEncRows; ++i) {
                const float d0 = r[i][j] - w.x, d1 = r[i][j + 1] - w.y;
                acc[i] = __builtin_fmaf(d0, d0, acc[i]);
                acc[i] = __builtin_fmaf(d1, d1, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kEncRows; ++i) {
            if (acc[i] < best[i]) {  // strict: the lowest codeword wins ties
                best[i] = acc[i];
                code[i] = c;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kEncRows; ++i)
        if (row[i] < n) codes[row[i] * M + m] = static_cast<uint8_t>(code[i]);
}

// ---- the tables ----
constexpr int kLutGroup = 4;  // subspaces per block

__global__ __launch_bounds__(kCodewords) void pq_tables(const float* __restrict__ Q, int d, int M, int dsub,
                                                        const float* __restrict__ codebooks, float* __restrict__ lut) {
    __shared__ __attribute__((aligned(16))) float qs[kLutGroup * kMaxDsub];
    const int q = blockIdx.x, m0 = blockIdx.y * kLutGroup, c = threadIdx.x;
    const int span = kLutGroup * dsub;  // M % 4 == 0: the group is whole
    if (c < span) qs[c] = Q[static_cast<int64_t>(q) * d + m0 * dsub + c];
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kLutGroup; ++g) {
        const int m = m0 + g;
        const float* w = codebooks + (static_cast<int64_t>(m) * kCodewords + c) * dsub;
        float acc = 0.f;
        for (int j = 0; j < dsub; j += 2) {
            const float2 wv = *reinterpret_cast<const float2*>(w + j);
            const float2 qv = *reinterpret_cast<const float2*>(qs + g * dsub + j);
            acc = __builtin_fmaf(qv.x, wv.x, acc);
            acc = __builtin_fmaf(qv.y, wv.y, acc);
        }
        lut[(static_cast<int64_t>(q) * M + m) * kCodewords + c] = acc;
    }
}

// ---- the scan ----

// LDS of a scan block: the query's table (MCAP KB), the candidate buffer and
// the compaction's histograms. No row stage.
template <int MCAP>
struct Lds {
    static constexpr int kTable = MCAP * kCodewords * 4;
    static constexpr int kWords = MCAP / 4;  // 4-byte words of a row's codes, at most
    // blocks per CU the launch bounds ask for: what the LDS takes, at most 4 (128 VGPRs)
    static constexpr int kBlocks = MCAP > 32 ? 2 : 4;
    static constexpr int kCand = on::kCap * static_cast<int>(sizeof(Cand));
    static constexpr int kHist = on::kWavesS * 256 * 4;
    static constexpr int kBytes = kTable + kCand + kHist;
    static_assert(kTable % 16 == 0 && kCand % 16 == 0, "ivf_pq: 16-byte aligned regions");
    // 384: cnt and thr, the scratch of the block-wide reduction, alignment (ivf.hip's kListSlack)
    static_assert(kBlocks * (kBytes + 384 + 128) <= 163840, "ivf_pq: kBlocks blocks per CU (two at M = 64)");
};
static_assert(Lds<kMaxM>::kBytes == 65536 + 3584 + 4096, "ivf_pq: 64 KB of table and 7.5 KB of selection state");

// the M code bytes of stored row `row` as 4-byte words: 16-byte loads when M % 16 == 0
template <int NW>
__device__ __forceinline__ void load_codes(uint32_t (&W)[NW], const uint8_t* __restrict__ codes, int64_t row, int M,
                                           bool valid) {
    const uint8_t* p = codes + row * M;
    if ((M & 15) == 0) {  // block-uniform
#pragma unroll
        for (int u = 0; u < NW / 4; ++u) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (u * 16 < M && valid) v = *reinterpret_cast<const uint4*>(p + u * 16);
            W[4 * u] = v.x;
            W[4 * u + 1] = v.y;
            W[4 * u + 2] = v.z;
            W[4 * u + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            W[i] = 0u;
            if (i * 4 < M && valid) W[i] = *reinterpret_cast<const uint32_t*>(p + i * 4);
        }
    }
}

template <int MCAP>
__global__ __launch_bounds__(on::kThreads, Lds<MCAP>::kBlocks) void ivf_pq_scan(
    const float* __restrict__ lut, const uint8_t* __restrict__ codes, int64_t nx, int M, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int32_t* __restrict__ row_pos,
    const int64_t* __restrict__ probes, const float* __restrict__ bias, int nprobe, int chunks,
    int64_t rows_per_chunk, const uint32_t* __restrict__ excl, int64_t excl_words, uint64_t* __restrict__ partials) {
    constexpr int kThreads = on::kThreads, kTileRows = on::kTileRows;
    using L = Lds<MCAP>;
    __shared__ __attribute__((aligned(16))) char lds[L::kBytes];
    __shared__ int cnt;
    __shared__ float thr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lists = nprobe * chunks;
    const int lb = blockIdx.x, q = blockIdx.y;
    const int p = lb / chunks, c = lb - p * chunks;
    uint64_t* const out = partials + static_cast<int64_t>(q) * k * lists + lb;  // [q][rank][lb]

    int64_t row_begin, row_end;
    iv::chunk_window(probes[static_cast<int64_t>(q) * nprobe + p], c, list_offsets, nlist, nullptr, nx, rows_per_chunk,
                     row_begin, row_end);
    if (row_end <= row_begin) {  // block-uniform
        iv::write_none(out, k, lists);
        return;
    }
    const int tiles = static_cast<int>((row_end - row_begin + kTileRows - 1) / kTileRows);

    // tile 0's codes and positions, in flight under the table copy
    constexpr int NW = L::kWords;
    uint32_t W[NW];
    int64_t row = row_begin + threadIdx.x;
    load_codes(W, codes, row, M, row < row_end);
    int32_t pos_next = row < row_end ? row_pos[row] : -1;

    float* const table = reinterpret_cast<float*>(lds);
    Cand* const cand = reinterpret_cast<Cand*>(lds + L::kTable);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + L::kTable + L::kCand) + wave * 256;
    const float4* src = reinterpret_cast<const float4*>(lut + static_cast<int64_t>(q) * M * kCodewords);
    for (int e = threadIdx.x; e < M * (kCodewords / 4); e += kThreads) reinterpret_cast<float4*>(table)[e] = src[e];
    const float b = bias ? bias[static_cast<int64_t>(q) * nprobe + p] : 0.f;
    if (threadIdx.x == 0) {
        cnt = 0;
        thr = -INFINITY;
    }
    __syncthreads();

    int over = 0;  // decided through the barrier that ends a tile: block-uniform (ivf_scan)
    for (int t = 0; t < tiles; ++t) {
        if (over) {
            if (wave == 0) {
                int n = cnt;
                float th = thr;
                iv::compact_keep_ties(cand, n, k, on::kRoom, hist, th);
                if (lane == 0) {
                    cnt = n;
                    thr = th;
                }
            }
            __syncthreads();
        }
        const float th = thr;
        const int32_t pos = pos_next;
        uint32_t C[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) C[i] = W[i];
        // the next tile's codes and position: issued before this tile's lookups
        row += kTileRows;
        load_codes(W, codes, row, M, row < row_end);
        pos_next = row < row_end ? row_pos[row] : -1;

        // a row past the window reads code 0 of every subspace: inside the table, never appended
        float acc = b;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i * 4 < M) {  // block-uniform
                const float* const tm = table + i * 4 * kCodewords;
                const float v0 = tm[C[i] & 0xFFu];
                const float v1 = tm[kCodewords + ((C[i] >> 8) & 0xFFu)];
                const float v2 = tm[2 * kCodewords + ((C[i] >> 16) & 0xFFu)];
                const float v3 = tm[3 * kCodewords + (C[i] >> 24)];
                acc = acc + v0;
                acc = acc + v1;
                acc = acc + v2;
                acc = acc + v3;
            }
        }

        // ---- selection: ivf_scan's, at most one append per row ----
        bool pass = iv::pos_passes(pos, nx, acc, th);
        if (excl && pass) pass = iv::bitmap_clear(excl, excl_words, q, pos);
        over = __syncthreads_or(on::append<true>(pass, &cnt, cand, acc, static_cast<uint32_t>(pos)));
    }

    if (wave == 0) on::write_block_list(cand, cnt, k, hist, out, lists);
}

inline bool m_ok(int d, int M) {
    if (M < kMinM || M > kMaxM || (M & 3) || d % M) return false;
    const int dsub = d / M;
    return (dsub & 1) == 0 && dsub <= kMaxDsub;
}

inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

}  // namespace ivfpq
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace pq = rt::topk::ivfpq;
namespace pqon = rt::topk::online;
namespace pqiv = rt::topk::ivf;

static_assert(RT_PQ_MAX_M == pq::kMaxM, "rtrec_hip.h restates the kernel's limits");

extern "C" int rt_pq_encode(const void* rows, int64_t n, int d, int dtype, const float* centroids, int64_t nlist,
                            const int64_t* assign, const float* codebooks, int M, uint8_t* codes, void* stream) {
    if (n < 0 || d <= 0 || M <= 0) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if ((centroids != nullptr) != (assign != nullptr) || (centroids && nlist <= 0)) return RT_ERR_INVALID;
    if (!pqon::shape_ok(d, dtype) || !pq::m_ok(d, M)) return RT_ERR_UNSUPPORTED;
    if (n == 0) return RT_OK;
    if (!rows || !codebooks || !codes) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(codebooks) |
         reinterpret_cast<uintptr_t>(centroids)) & 15)
        return RT_ERR_INVALID;
    if (n >= 0x7FFFFFFFll * pq::kEncTile) return RT_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const dim3 grid(static_cast<unsigned>((n + pq::kEncTile - 1) / pq::kEncTile), static_cast<unsigned>(M));
    const dim3 block(pq::kEncThreads);
#define RT_PQ_ENCODE(DSUB)                                                                                       \
    case DSUB:                                                                                                   \
        hipLaunchKernelGGL((pq::pq_encode<DSUB>), grid, block, 0, st, rows, n, d, dtype, centroids, nlist, assign, \
                           codebooks, M, codes);                                                                 \
        break
    switch (d / M) {
        RT_PQ_ENCODE(2);
        RT_PQ_ENCODE(4);
        RT_PQ_ENCODE(6);
        RT_PQ_ENCODE(8);
        RT_PQ_ENCODE(10);
        RT_PQ_ENCODE(12);
        RT_PQ_ENCODE(14);
        RT_PQ_ENCODE(16);
        RT_PQ_ENCODE(18);
        RT_PQ_ENCODE(20);
        RT_PQ_ENCODE(22);
        RT_PQ_ENCODE(24);
        RT_PQ_ENCODE(26);
        RT_PQ_ENCODE(28);
        RT_PQ_ENCODE(30);
        default:
            RT_PQ_ENCODE(32);
    }
#undef RT_PQ_ENCODE
    return check_launch("pq_encode");
}

// the partial lists of rt_ivf_topk, then the tables [nq][M][256] fp32
extern "C" size_t rt_ivf_pq_topk_workspace_bytes(int64_t nq, int nprobe, int64_t max_list_rows, int k, int M) {
    if (nq <= 0 || M < pq::kMinM || M > pq::kMaxM || (M & 3)) return 256;
    return pq::align256(rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k)) +
           static_cast<size_t>(nq) * M * pq::kCodewords * sizeof(float);
}

extern "C" int rt_ivf_pq_topk(const float* queries, int64_t nq, int d, const uint8_t* codes, int64_t nx, int M,
                              const float* codebooks, const int64_t* list_offsets, int64_t nlist,
                              const int32_t* row_pos, const int64_t* probes, const float* bias, int nprobe,
                              int64_t max_list_rows, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                              float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || M <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0)
        return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !codebooks || !out_scores || !out_ids || !list_offsets || !probes || (nx > 0 && (!codes || !row_pos)))
        return RT_ERR_INVALID;
    if (k > pqon::kMaxK || nprobe > pqiv::kMaxProbe || nq > pqiv::kMaxNq) return RT_ERR_UNSUPPORTED;
    if (!pqon::shape_ok(d, RT_F32) || !pq::m_ok(d, M)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll || max_list_rows >= 0xFFFFFFFFll) return RT_ERR_UNSUPPORTED;  // positions are int32
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(codebooks) |
         reinterpret_cast<uintptr_t>(codes)) & 15)
        return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(bias) & 3) || (exclude_bits && exclude_words < (nx + 31) / 32))
        return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < rt_ivf_pq_topk_workspace_bytes(nq, nprobe, max_list_rows, k, M))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return RT_ERR_INVALID;
    int64_t plan[3];
    if (rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK) return RT_ERR_UNSUPPORTED;
    const int chunks = static_cast<int>(plan[0]);
    const int64_t rows_per_chunk = plan[1];
    const int lists = nprobe * chunks;
    hipStream_t st = as_stream(stream);
    uint64_t* partials = static_cast<uint64_t*>(workspace);
    float* lut = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                          pq::align256(rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k)));

    hipLaunchKernelGGL(pq::pq_tables, dim3(static_cast<unsigned>(nq), static_cast<unsigned>(M / pq::kLutGroup)),
                       dim3(pq::kCodewords), 0, st, queries, d, M, d / M, codebooks, lut);
    int rc = check_launch("pq_tables");
    if (rc) return rc;

    const dim3 grid(static_cast<unsigned>(lists), static_cast<unsigned>(nq)), block(pqon::kThreads);
#define RT_IVF_PQ_LAUNCH(MCAP)                                                                                    \
    hipLaunchKernelGGL((pq::ivf_pq_scan<MCAP>), grid, block, 0, st, lut, codes, nx, M, k, list_offsets, nlist,    \
                       row_pos, probes, bias, nprobe, chunks, rows_per_chunk, exclude_bits, exclude_words, partials)
    if (M <= 16) RT_IVF_PQ_LAUNCH(16);
    else if (M <= 32) RT_IVF_PQ_LAUNCH(32);
    else RT_IVF_PQ_LAUNCH(64);
#undef RT_IVF_PQ_LAUNCH
    rc = check_launch("ivf_pq_scan");
    if (rc) return rc;
    return pqon::launch_finish(partials, lists, k, out_scores, out_ids, 0, nq, st);
}
