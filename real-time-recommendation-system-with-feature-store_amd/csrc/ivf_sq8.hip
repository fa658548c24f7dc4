// IVF-SQ8: 8-bit scalar-quantised lists (faiss.index_factory(d, "IVF1024,SQ8"),
// the factory string of src/serving/retrieval.py:96-110). A row is d bytes:
// code_j names one of 256 bins of dimension j's range, decoded as
// lo_j + (code_j + 0.5) step_j. The third row format of the probed-list scan,
// next to the rows of ivf.hip and the PQ codes of ivf_pq.hip.
//
// rt_sq8_encode, one launch: a thread owns 4 consecutive elements of one row
// and writes their codes as one 4-byte word. Consecutive threads read
// consecutive 16 (fp32) or 8 (f16 / bf16) bytes of the rows and write
// consecutive words: both streams are coalesced, no lane walks a row. lo and
// inv_step are float4 reads that every row of a block repeats (cache hits),
// the centroid of a residual a float4 gather by the row's list. t = (r - lo)
// * inv_step, one subtraction and one multiplication; the code is 255 for
// t >= 255, (int)t for t > 0, else 0 (NaN included).
//
// rt_ivf_sq8_topk, three launches (no host read, stream-ordered, capturable):
//
// 1. sq8_fold, one block per query: the quantiser is folded into the query.
//    qs[j] = q_j step_j and base[p] = bias[p] + b0, b0 = sum_j q_j mid_j with
//    mid_j = fmaf(0.5, step_j, lo_j), one thread's sequential fmaf chain from 0
//    (d dependent FMAs: paid once per query here, not once per scan block).
//    A row's score is then base[p] + sum_j qs[j] code_j: no subtraction of lo
//    and no multiplication by step per element.
// 2. ivf_sq8_scan: rt_ivf_topk's grid (probe x chunk, query), its window and
//    everything behind the score (ivf_select.h). Rows move as in the online
//    scan (topk_online.h: load_step, coalesced 16-byte loads into registers,
//    then the wave's LDS stage with rows padded to 144 B, lane = row), but a
//    16-byte unit now carries 16 dimensions: one 8-unit step covers d = 128,
//    so for d <= 128 a tile is one step and the global loads of tile t + 1 are
//    in flight under all of tile t's arithmetic. Per unit a lane reads its 16
//    bytes (one ds_read_b128, conflict-free by the padding) and four float4 of
//    qs (wave-uniform broadcasts), widens each byte with v_cvt_f32_ubyte0..3
//    and runs acc = fmaf(qs[j], code_j, acc), j ascending, from acc = base[p].
//    No dot or matrix instruction: the sequential chain is the contract.
//    LDS is the online scan's Lds<1> (45,568 B): three blocks per CU.
// 3. flatip_online_finish (topk_online.h, unchanged).
#include "ivf_select.h"
#include "ivf_sq8_fold.h"

namespace rt {
namespace topk {
namespace ivfsq8 {

namespace on = rt::topk::online;
namespace iv = rt::topk::ivf;

// ---- rt_sq8_encode ----
constexpr int kEncThreads = 256;

__device__ __forceinline__ float4 load4(const void* rows, int dtype, int64_t e) {  // e % 4 == 0
    if (dtype == RT_F32) return *reinterpret_cast<const float4*>(static_cast<const float*>(rows) + e);
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(rows) + e);
    const uint16_t h0 = static_cast<uint16_t>(v.x & 0xFFFFu), h1 = static_cast<uint16_t>(v.x >> 16);
    const uint16_t h2 = static_cast<uint16_t>(v.y & 0xFFFFu), h3 = static_cast<uint16_t>(v.y >> 16);
    if (dtype == RT_F16)
        return make_float4(bits_f16_to_f32(h0), bits_f16_to_f32(h1), bits_f16_to_f32(h2), bits_f16_to_f32(h3));
    return make_float4(bits_bf16_to_f32(h0), bits_bf16_to_f32(h1), bits_bf16_to_f32(h2), bits_bf16_to_f32(h3));
}

__device__ __forceinline__ uint32_t code_of(float r, float lo, float inv) {
    const float t = (r - lo) * inv;
    if (t >= 255.f) return 255u;
    return t > 0.f ? static_cast<uint32_t>(static_cast<int>(t)) : 0u;  // NaN: 0
}

__global__ __launch_bounds__(kEncThreads) void sq8_encode(const void* __restrict__ rows, int64_t words, int d,
                                                          int dtype, const float* __restrict__ centroids,
                                                          int64_t nlist, const int64_t* __restrict__ assign,
                                                          const float* __restrict__ lo,
                                                          const float* __restrict__ inv_step,
                                                          uint32_t* __restrict__ codes) {
    const int64_t w = static_cast<int64_t>(blockIdx.x) * kEncThreads + threadIdx.x;  // word of the code image
    if (w >= words) return;
    const int wpr = d >> 2;  // words per row
    const int64_t row = w / wpr;
    const int j = static_cast<int>(w - row * wpr) * 4;
    float4 x = load4(rows, dtype, w * 4);
    if (centroids) {
        const int64_t l = assign[row];
        if (l >= 0 && l < nlist) {
            const float4 c = *reinterpret_cast<const float4*>(centroids + l * d + j);
            x.x = x.x - c.x;
            x.y = x.y - c.y;
            x.z = x.z - c.z;
            x.w = x.w - c.w;
        }
    }
    const float4 a = *reinterpret_cast<const float4*>(lo + j);
    const float4 s = *reinterpret_cast<const float4*>(inv_step + j);
    codes[w] = code_of(x.x, a.x, s.x) | (code_of(x.y, a.y, s.y) << 8) | (code_of(x.z, a.z, s.z) << 16) |
               (code_of(x.w, a.w, s.w) << 24);
}

// ---- the fold ----
constexpr int kFoldThreads = 256;
static_assert(kFoldThreads >= kMaxD && kFoldThreads >= iv::kMaxProbe, "sq8_fold: a thread per dimension and per probe");

__global__ __launch_bounds__(kFoldThreads) void sq8_fold(const float* __restrict__ Q, int d,
                                                         const float* __restrict__ lo, const float* __restrict__ step,
                                                         const float* __restrict__ bias, int nprobe, int stride,
                                                         float* __restrict__ fold) {
    __shared__ float qv[kMaxD], mid[kMaxD];
    __shared__ float b0;
    const int q = blockIdx.x, t = threadIdx.x;
    float* const out = fold + static_cast<int64_t>(q) * stride;
    if (t < d) {
        const float x = Q[static_cast<int64_t>(q) * d + t], s = step[t];
        qv[t] = x;
        mid[t] = __builtin_fmaf(0.5f, s, lo[t]);
        out[t] = x * s;
    }
    __syncthreads();
    if (t == 0) {
        float acc = 0.f;
        for (int j = 0; j < d; ++j) acc = __builtin_fmaf(qv[j], mid[j], acc);
        b0 = acc;
    }
    __syncthreads();
    if (t < nprobe) out[d + t] = bias ? bias[static_cast<int64_t>(q) * nprobe + t] + b0 : b0;
}

int launch_fold(const float* queries, int64_t nq, int d, const float* lo, const float* step, const float* bias,
                int nprobe, int stride, float* fold, hipStream_t st) {
    hipLaunchKernelGGL(sq8_fold, dim3(static_cast<unsigned>(nq)), dim3(kFoldThreads), 0, st, queries, d, lo, step,
                       bias, nprobe, stride, fold);
    return check_launch("sq8_fold");
}

// ---- the scan ----
using L = on::Lds<1>;  // the wave stages, the candidate buffer, the query (qs), the histograms
constexpr int kBlocks = 3;  // per CU: 12 waves, 3 per SIMD, <= 168 VGPRs
// 384: cnt and thr, the scratch of the block-wide reduction, alignment (ivf.hip's kListSlack)
static_assert(kBlocks * (L::kBytes + 384 + 128) <= 163840, "ivf_sq8: three blocks per CU");
static_assert(L::kQuery >= kMaxD * 4, "ivf_sq8: qs takes the query's region");

// Staged score chain of one tile for this lane's row (the wave's 64-row group,
// lane = row), from acc = base. R holds the tile's first step on entry
// (on::load_step) and the next tile's first step on return.
__device__ __forceinline__ float score_tile(uint4 (&R)[on::kStepUnits], const on::RowWindow& w, int t, char* stage,
                                            const float* qs, float acc) {
    constexpr int kStepUnits = on::kStepUnits, kRowStride = on::kRowStride;
    const int lane = threadIdx.x & 63;
    for (int c = 0; c < w.steps; ++c) {
#pragma unroll
        for (int i = 0; i < kStepUnits; ++i) {
            const int f = i * 64 + lane;
            *reinterpret_cast<uint4*>(stage + (f >> 3) * kRowStride + (f & 7) * 16) = R[i];
        }
        if (c + 1 < w.steps) on::load_step(R, w, t, c + 1);
        else on::load_step(R, w, t + 1, 0);
        wave_lds_sync();
        const int nu = (w.units - c * kStepUnits) < kStepUnits ? (w.units - c * kStepUnits) : kStepUnits;
#pragma unroll
        for (int u = 0; u < kStepUnits; ++u) {
            if (u >= nu) break;  // wave-uniform
            const uint4 xv = *reinterpret_cast<const uint4*>(stage + lane * kRowStride + u * 16);
            const uint32_t x[4] = {xv.x, xv.y, xv.z, xv.w};
            const int j0 = (c * kStepUnits + u) * 16;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float4 qv = *reinterpret_cast<const float4*>(qs + j0 + 4 * h);
                acc = __builtin_fmaf(qv.x, static_cast<float>(x[h] & 0xFFu), acc);
                acc = __builtin_fmaf(qv.y, static_cast<float>((x[h] >> 8) & 0xFFu), acc);
                acc = __builtin_fmaf(qv.z, static_cast<float>((x[h] >> 16) & 0xFFu), acc);
                acc = __builtin_fmaf(qv.w, static_cast<float>((x[h] >> 24) & 0xFFu), acc);
            }
        }
        wave_lds_sync();  // the stage is rewritten by the next step
    }
    return acc;
}

__global__ __launch_bounds__(on::kThreads, kBlocks) void ivf_sq8_scan(
    const float* __restrict__ fold, int stride, const char* __restrict__ codes, int64_t nx, int d, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int32_t* __restrict__ row_pos,
    const int64_t* __restrict__ probes, int nprobe, int chunks, int64_t rows_per_chunk,
    const uint32_t* __restrict__ excl, int64_t excl_words, uint64_t* __restrict__ partials) {
    constexpr int kTileRows = on::kTileRows, kStepUnits = on::kStepUnits;
    __shared__ __attribute__((aligned(16))) char lds[L::kBytes];
    __shared__ int cnt;
    __shared__ float thr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lists = nprobe * chunks;
    const int lb = blockIdx.x, q = blockIdx.y;
    const int p = lb / chunks, c = lb - p * chunks;
    uint64_t* const out = partials + static_cast<int64_t>(q) * k * lists + lb;  // [q][rank][lb]

    on::RowWindow w;
    w.X = codes;
    iv::chunk_window(probes[static_cast<int64_t>(q) * nprobe + p], c, list_offsets, nlist, nullptr, nx, rows_per_chunk,
                     w.row_begin, w.row_end);
    if (w.row_end <= w.row_begin) {  // block-uniform
        iv::write_none(out, k, lists);
        return;
    }
    w.units = d >> 4;
    w.row_bytes = d;
    w.steps = (w.units + kStepUnits - 1) / kStepUnits;
    w.tiles = static_cast<int>((w.row_end - w.row_begin + kTileRows - 1) / kTileRows);

    // tile 0's codes and positions, in flight under the copy of the folded query
    uint4 R[kStepUnits];
    on::load_step(R, w, 0, 0);
    int64_t row = w.row_begin + threadIdx.x;
    int32_t pos_next = row < w.row_end ? row_pos[row] : -1;

    char* const stage = lds + wave * on::kStageBytes;
    Cand* const cand = reinterpret_cast<Cand*>(lds + L::kStage);
    float* const qs = reinterpret_cast<float*>(lds + L::kStage + L::kCand);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + L::kStage + L::kCand + L::kQuery) + wave * 256;
    const float* const mine = fold + static_cast<int64_t>(q) * stride;
    if (threadIdx.x < (d >> 2))
        reinterpret_cast<float4*>(qs)[threadIdx.x] = reinterpret_cast<const float4*>(mine)[threadIdx.x];
    const float base = mine[d + p];
    if (threadIdx.x == 0) {
        cnt = 0;
        thr = -INFINITY;
    }
    __syncthreads();

    int over = 0;  // decided through the barrier that ends a tile: block-uniform (ivf_scan)
    for (int t = 0; t < w.tiles; ++t) {
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
        row += kTileRows;
        pos_next = row < w.row_end ? row_pos[row] : -1;

        // a row past the window is staged as zeros: code 0 everywhere, never appended (pos = -1)
        const float acc = score_tile(R, w, t, stage, qs, base);

        // ---- selection: ivf_scan's, at most one append per row ----
        bool pass = iv::pos_passes(pos, nx, acc, th);
        if (excl && pass) pass = iv::bitmap_clear(excl, excl_words, q, pos);
        over = __syncthreads_or(on::append<true>(pass, &cnt, cand, acc, static_cast<uint32_t>(pos)));
    }

    if (wave == 0) on::write_block_list(cand, cnt, k, hist, out, lists);
}

}  // namespace ivfsq8
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace sq = rt::topk::ivfsq8;
namespace sqon = rt::topk::online;
namespace sqiv = rt::topk::ivf;

static_assert(RT_SQ8_MIN_D == sq::kMinD && RT_SQ8_MAX_D == sq::kMaxD, "rtrec_hip.h restates the kernel's limits");

extern "C" int rt_sq8_encode(const void* rows, int64_t n, int d, int dtype, const float* centroids, int64_t nlist,
                             const int64_t* assign, const float* lo, const float* inv_step, uint8_t* codes,
                             void* stream) {
    if (n < 0 || d <= 0) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if ((centroids != nullptr) != (assign != nullptr) || (centroids && nlist <= 0)) return RT_ERR_INVALID;
    if (!sq::d_ok(d)) return RT_ERR_UNSUPPORTED;
    if (n == 0) return RT_OK;
    if (!rows || !lo || !inv_step || !codes) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(inv_step) |
         reinterpret_cast<uintptr_t>(centroids) | reinterpret_cast<uintptr_t>(codes)) & 15)
        return RT_ERR_INVALID;
    if (n >= 0x7FFFFFFFll * sq::kEncThreads / (d >> 2)) return RT_ERR_UNSUPPORTED;  // grid.x
    const int64_t words = n * (d >> 2);
    const int64_t blocks = (words + sq::kEncThreads - 1) / sq::kEncThreads;
    hipLaunchKernelGGL(sq::sq8_encode, dim3(static_cast<unsigned>(blocks)), dim3(sq::kEncThreads), 0,
                       as_stream(stream), rows, words, d, dtype, centroids, nlist, assign, lo, inv_step,
                       reinterpret_cast<uint32_t*>(codes));
    return check_launch("sq8_encode");
}

// the partial lists of rt_ivf_topk, then the folded queries [nq][d + nprobe padded to 4] fp32
extern "C" size_t rt_ivf_sq8_topk_workspace_bytes(int64_t nq, int nprobe, int64_t max_list_rows, int k, int d) {
    int64_t plan[3];
    if (k <= 0 || k > sqon::kMaxK || !sq::d_ok(d) || rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK)
        return 256;
    return sq::align256(rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k)) +
           static_cast<size_t>(nq) * sq::fold_stride(d, nprobe) * sizeof(float);
}

extern "C" int rt_ivf_sq8_topk(const float* queries, int64_t nq, int d, const uint8_t* codes, int64_t nx,
                               const float* lo, const float* step, const int64_t* list_offsets, int64_t nlist,
                               const int32_t* row_pos, const int64_t* probes, const float* bias, int nprobe,
                               int64_t max_list_rows, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                               float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !lo || !step || !out_scores || !out_ids || !list_offsets || !probes ||
        (nx > 0 && (!codes || !row_pos)))
        return RT_ERR_INVALID;
    if (k > sqon::kMaxK || nprobe > sqiv::kMaxProbe || nq > sqiv::kMaxNq) return RT_ERR_UNSUPPORTED;
    if (!sq::d_ok(d)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll || max_list_rows >= 0xFFFFFFFFll) return RT_ERR_UNSUPPORTED;  // positions are int32
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(step) |
         reinterpret_cast<uintptr_t>(codes)) & 15)
        return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(bias) & 3) || (exclude_bits && exclude_words < (nx + 31) / 32))
        return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < rt_ivf_sq8_topk_workspace_bytes(nq, nprobe, max_list_rows, k, d))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return RT_ERR_INVALID;
    int64_t plan[3];
    if (rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK) return RT_ERR_UNSUPPORTED;
    const int chunks = static_cast<int>(plan[0]);
    const int64_t rows_per_chunk = plan[1];
    const int lists = nprobe * chunks;
    const int stride = sq::fold_stride(d, nprobe);
    hipStream_t st = as_stream(stream);
    uint64_t* partials = static_cast<uint64_t*>(workspace);
    float* fold = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                           sq::align256(rt_ivf_topk_workspace_bytes(nq, nprobe, max_list_rows, k)));

    int rc = sq::launch_fold(queries, nq, d, lo, step, bias, nprobe, stride, fold, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sq::ivf_sq8_scan, dim3(static_cast<unsigned>(lists), static_cast<unsigned>(nq)),
                       dim3(sqon::kThreads), 0, st, fold, stride, reinterpret_cast<const char*>(codes), nx, d, k,
                       list_offsets, nlist, row_pos, probes, nprobe, chunks, rows_per_chunk, exclude_bits,
                       exclude_words, partials);
    rc = check_launch("ivf_sq8_scan");
    if (rc) return rc;
    return sqon::launch_finish(partials, lists, k, out_scores, out_ids, 0, nq, st);
}
