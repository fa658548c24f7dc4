// rt_refine_topk: exact re-rank of an over-fetch (Faiss's IndexRefine: "IVF1024,
// PQ16,RFlat" / "IVF1024,PQ16,Refine(SQ8)"). Per query up to 128 candidate
// positions, as rt_ivf_pq_topk wrote them, are scored against a row store held
// in ORIGINAL position order (fp32 / f16 / bf16 rows, or non-residual SQ8
// codes) and the best k are written. One launch, no workspace, no host read.
//
// The work is a random gather of nq x n_cand rows of 128-1024 B with no reuse
// of a row across queries, and every score is ONE sequential fmaf chain (the
// contract of rt_flatip_topk and rt_ivf_sq8_topk). So: no MFMA (nothing to
// amortise over <= 128 rows, and one chain per score), no split of a row's sum
// across lanes. What the kernel is built around is the gather.
//
// Split: one workgroup per query, one LANE per candidate, so a wave owns 64
// candidates and the block is ceil(n_cand / 64) <= 2 waves. Rows move as in the
// online and SQ8 scans: in k-steps of 8 sixteen-byte units (128 B of every
// row), consecutive lanes load consecutive units of one row — 8 lanes per row,
// 8 rows per load instruction, 8 instructions per step for the wave's 64 rows;
// a lane learns the position of the row it loads for by a shuffle from the lane
// that owns that candidate. The 8 loads of step c + 1 are issued into registers
// before the arithmetic of step c starts, so the gather latency of a step hides
// under the 32-128 dependent FMAs of the one before it, and under the other
// blocks of the CU. An absent candidate (id < 0 or >= n_rows) is never read.
//
// LDS: per wave a stage of 64 rows x 144 B (128 B of data, 16 B of padding: a
// lane's ds_read_b128 of its own row is conflict-free), the query as fp32
// (SQ8: qs = q * step, and q and mid for the b0 chain), and the 128 (key,
// position) pairs of the selection: 20,992 B (23,040 B for SQ8), 7 blocks per
// CU. The stage is private to its wave: the k-loop has no barrier.
//
// Scores: row stores acc = fmaf(q_j, (float)x_j, acc) from 0, j ascending — with
// an fp32 store rt_flatip_topk's bits. SQ8: sq8_fold's arithmetic restated in
// the kernel (one launch, no workspace for a fold): mid_j = fmaf(0.5, step_j,
// lo_j), b0 = the chain fmaf(q_j, mid_j, .) from 0, qs_j = q_j * step_j, then
// acc = fmaf(qs_j, (float)code_j, acc) from b0; bytes widen with
// v_cvt_f32_ubyte0..3. Every lane runs the b0 chain itself from LDS broadcasts
// while its first step's loads are in flight.
//
// Selection: rank by counting over the <= 128 (key, position, index) triples in
// LDS, key = the score's bits mapped to an unsigned total order (-0 counts as
// +0, a NaN orders by its bits): ranks are a permutation, so no two candidates
// claim one slot. A present candidate of rank < k writes slot rank; the slots
// from the present count to k get (-FLT_MAX, -1).
#include <float.h>

#include "ivf_sq8_fold.h"
#include "rt_common.h"

namespace rt {
namespace refine {

constexpr int kMaxCand = RT_REFINE_MAX_CAND;
constexpr int kMaxWaves = kMaxCand / RT_WAVE;       // 2
constexpr int kThreads = kMaxCand;                  // a lane per candidate
constexpr int kStepUnits = 8;                       // 16-byte units of a row per k-step
constexpr int kRowStride = kStepUnits * 16 + 16;    // 144: bank-conflict-free b128 row reads
constexpr int kStageBytes = RT_WAVE * kRowStride;   // 9,216 per wave
constexpr int kMaxD = 256;
constexpr int64_t kMaxNq = 65535;
constexpr int kBlocksPerCU = 7;

template <int KIND>
struct Lds {
    static constexpr int kStage = 0;
    static constexpr int kQuery = kStage + kMaxWaves * kStageBytes;   // fp32 [kMaxD]: q, or qs for SQ8
    static constexpr int kPos = kQuery + kMaxD * 4;                   // int64 [kMaxCand]
    static constexpr int kKey = kPos + kMaxCand * 8;                  // uint32 [kMaxCand]
    static constexpr int kFold = kKey + kMaxCand * 4;                 // SQ8: q and mid, fp32 [kMaxD] each
    static constexpr int kBytes = kFold + (KIND == RT_REFINE_SQ8 ? 2 * kMaxD * 4 : 0);
};
static_assert(kBlocksPerCU * Lds<RT_REFINE_SQ8>::kBytes <= 163840, "refine: seven blocks per CU");
static_assert(kMaxWaves * RT_WAVE == kMaxCand, "refine: a lane per candidate");

template <int KIND>
struct Unit;   // 16 bytes of a stored row against the query elements they meet
template <>
struct Unit<RT_F32> {
    static constexpr int kElems = 4;
    __device__ static __forceinline__ float dot(const uint4& x, const float* q, float acc) {
        const float4 a = *reinterpret_cast<const float4*>(q);
        acc = __builtin_fmaf(a.x, __uint_as_float(x.x), acc);
        acc = __builtin_fmaf(a.y, __uint_as_float(x.y), acc);
        acc = __builtin_fmaf(a.z, __uint_as_float(x.z), acc);
        acc = __builtin_fmaf(a.w, __uint_as_float(x.w), acc);
        return acc;
    }
};
template <bool BF>
__device__ __forceinline__ float widen_lo(uint32_t w) {
    return BF ? __uint_as_float(w << 16) : bits_f16_to_f32(static_cast<uint16_t>(w & 0xFFFFu));
}
template <bool BF>
__device__ __forceinline__ float widen_hi(uint32_t w) {
    return BF ? __uint_as_float(w & 0xFFFF0000u) : bits_f16_to_f32(static_cast<uint16_t>(w >> 16));
}
template <bool BF>
__device__ __forceinline__ float dot16(const uint4& x, const float* q, float acc) {
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    acc = __builtin_fmaf(a.x, widen_lo<BF>(x.x), acc);
    acc = __builtin_fmaf(a.y, widen_hi<BF>(x.x), acc);
    acc = __builtin_fmaf(a.z, widen_lo<BF>(x.y), acc);
    acc = __builtin_fmaf(a.w, widen_hi<BF>(x.y), acc);
    acc = __builtin_fmaf(b.x, widen_lo<BF>(x.z), acc);
    acc = __builtin_fmaf(b.y, widen_hi<BF>(x.z), acc);
    acc = __builtin_fmaf(b.z, widen_lo<BF>(x.w), acc);
    acc = __builtin_fmaf(b.w, widen_hi<BF>(x.w), acc);
    return acc;
}
template <>
struct Unit<RT_F16> {
    static constexpr int kElems = 8;
    __device__ static __forceinline__ float dot(const uint4& x, const float* q, float acc) {
        return dot16<false>(x, q, acc);
    }
};
template <>
struct Unit<RT_BF16> {
    static constexpr int kElems = 8;
    __device__ static __forceinline__ float dot(const uint4& x, const float* q, float acc) {
        return dot16<true>(x, q, acc);
    }
};
template <>
struct Unit<RT_REFINE_SQ8> {
    static constexpr int kElems = 16;
    __device__ static __forceinline__ float dot(const uint4& xv, const float* qs, float acc) {
        const uint32_t x[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const float4 a = *reinterpret_cast<const float4*>(qs + 4 * h);
            acc = __builtin_fmaf(a.x, static_cast<float>(x[h] & 0xFFu), acc);
            acc = __builtin_fmaf(a.y, static_cast<float>((x[h] >> 8) & 0xFFu), acc);
            acc = __builtin_fmaf(a.z, static_cast<float>((x[h] >> 16) & 0xFFu), acc);
            acc = __builtin_fmaf(a.w, static_cast<float>((x[h] >> 24) & 0xFFu), acc);
        }
        return acc;
    }
};

// the score's bits as an unsigned key of a total order; -0 is +0, as in a float comparison
__device__ __forceinline__ uint32_t order_key(float s) {
    const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The wave's loads of k-step c: lane l carries unit c * 8 + (l & 7) of the rows 8 i + (l >> 3),
// i = 0..7, of its wave's 64 candidates. src[i] is that row's first byte plus (l & 7) * 16, or
// NULL for an absent candidate; a unit past the row is not read. What is not read is zero.
__device__ __forceinline__ void load_step(uint4 (&R)[kStepUnits], const char* const (&src)[kStepUnits], int c,
                                          int units) {
    const bool in_row = c * kStepUnits + static_cast<int>(threadIdx.x & 7) < units;
#pragma unroll
    for (int i = 0; i < kStepUnits; ++i) {
        R[i] = make_uint4(0u, 0u, 0u, 0u);
        if (in_row && src[i]) R[i] = *reinterpret_cast<const uint4*>(src[i] + c * (kStepUnits * 16));
    }
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void refine_kernel(const float* __restrict__ Q, int d,
                                                          const int64_t* __restrict__ cand_ids, int n_cand,
                                                          const char* __restrict__ store, int64_t n_rows,
                                                          const float* __restrict__ lo,
                                                          const float* __restrict__ step, int k,
                                                          float* __restrict__ out_scores,
                                                          int64_t* __restrict__ out_ids) {
    using L = Lds<KIND>;
    using U = Unit<KIND>;
    __shared__ __attribute__((aligned(16))) char lds[L::kBytes];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int me = threadIdx.x;   // my candidate
    const int64_t q = blockIdx.x;

    int64_t id = -1;   // my candidate's position; -1 = absent
    if (me < n_cand) {
        id = cand_ids[q * n_cand + me];
        if (id < 0 || id >= n_rows) id = -1;
    }

    // ---- whose rows my loads carry, and step 0 in flight under the staging of the query ----
    const int units = d / U::kElems;
    const int64_t row_bytes = static_cast<int64_t>(units) * 16;
    const char* src[kStepUnits];
#pragma unroll
    for (int i = 0; i < kStepUnits; ++i) {
        const long long rid = __shfl(static_cast<long long>(id), i * 8 + (lane >> 3), 64);
        src[i] = rid >= 0 ? store + rid * row_bytes + (lane & 7) * 16 : nullptr;
    }
    uint4 R[kStepUnits];
    load_step(R, src, 0, units);

    float* const qv = reinterpret_cast<float*>(lds + L::kQuery);
    float* const q_raw = reinterpret_cast<float*>(lds + L::kFold);
    float* const mid = q_raw + kMaxD;
    for (int j = me; j < d; j += blockDim.x) {
        const float x = Q[q * d + j];
        if (KIND == RT_REFINE_SQ8) {
            const float s = step[j];
            q_raw[j] = x;
            mid[j] = __builtin_fmaf(0.5f, s, lo[j]);
            qv[j] = x * s;
        } else {
            qv[j] = x;
        }
    }
    __syncthreads();

    float acc = 0.f;
    if (KIND == RT_REFINE_SQ8) {   // b0: sq8_fold's chain, run by every lane from broadcasts
        for (int j = 0; j < d; j += 4) {
            const float4 a = *reinterpret_cast<const float4*>(q_raw + j);
            const float4 m = *reinterpret_cast<const float4*>(mid + j);
            acc = __builtin_fmaf(a.x, m.x, acc);
            acc = __builtin_fmaf(a.y, m.y, acc);
            acc = __builtin_fmaf(a.z, m.z, acc);
            acc = __builtin_fmaf(a.w, m.w, acc);
        }
    }

    // ---- the k-loop: stage step c, issue step c + 1, score step c ----
    char* const stage = lds + L::kStage + wave * kStageBytes;
    const int steps = (units + kStepUnits - 1) / kStepUnits;
    for (int c = 0; c < steps; ++c) {
#pragma unroll
        for (int i = 0; i < kStepUnits; ++i) {
            const int f = i * 64 + lane;   // row f >> 3 of the wave, unit f & 7 of the step
            *reinterpret_cast<uint4*>(stage + (f >> 3) * kRowStride + (f & 7) * 16) = R[i];
        }
        if (c + 1 < steps) load_step(R, src, c + 1, units);
        wave_lds_sync();
        const int left = units - c * kStepUnits;
        const int nu = left < kStepUnits ? left : kStepUnits;
#pragma unroll
        for (int u = 0; u < kStepUnits; ++u) {
            if (u >= nu) break;   // block-uniform: a unit past the row meets no query element
            const uint4 xv = *reinterpret_cast<const uint4*>(stage + lane * kRowStride + u * 16);
            acc = U::dot(xv, qv + (c * kStepUnits + u) * U::kElems, acc);
        }
        wave_lds_sync();   // the stage is rewritten by the next step
    }

    // ---- selection: rank by counting over (key desc, position asc, index asc) ----
    int64_t* const pos_s = reinterpret_cast<int64_t*>(lds + L::kPos);
    uint32_t* const key_s = reinterpret_cast<uint32_t*>(lds + L::kKey);
    const uint32_t key = order_key(acc);
    pos_s[me] = id;
    key_s[me] = key;
    __syncthreads();
    int rank = 0, present = 0;
    for (int j = 0; j < n_cand; ++j) {
        const int64_t pj = pos_s[j];
        const uint32_t kj = key_s[j];
        if (pj < 0) continue;   // block-uniform
        ++present;
        rank += (kj > key || (kj == key && (pj < id || (pj == id && j < me)))) ? 1 : 0;
    }
    float* const os = out_scores + q * k;
    int64_t* const oi = out_ids + q * k;
    if (id >= 0 && rank < k) {
        os[rank] = acc;
        oi[rank] = id;
    }
    for (int p = present + me; p < k; p += blockDim.x) {
        os[p] = -FLT_MAX;
        oi[p] = -1;
    }
}

template <int KIND>
int launch(const float* queries, int64_t nq, int d, const int64_t* cand_ids, int n_cand, const void* store,
           int64_t n_rows, const float* lo, const float* step, int k, float* out_scores, int64_t* out_ids,
           hipStream_t st) {
    const int threads = (n_cand + RT_WAVE - 1) / RT_WAVE * RT_WAVE;
    hipLaunchKernelGGL(refine_kernel<KIND>, dim3(static_cast<unsigned>(nq)), dim3(threads), 0, st, queries, d,
                       cand_ids, n_cand, static_cast<const char*>(store), n_rows, lo, step, k, out_scores, out_ids);
    return check_launch("refine_kernel");
}

}  // namespace refine
}  // namespace rt

using namespace rt;

static_assert(RT_REFINE_F32 == RT_F32 && RT_REFINE_F16 == RT_F16 && RT_REFINE_BF16 == RT_BF16,
              "rtrec_hip.h: a row store's kind is its dtype code");
static_assert(RT_REFINE_MAX_CAND == RT_IVF_MAX_K, "rtrec_hip.h: the refine takes what the IVF scans return");

extern "C" int rt_refine_topk(const float* queries, int64_t nq, int d, const int64_t* cand_ids, int n_cand,
                              const void* store, int64_t n_rows, int kind, const float* lo, const float* step, int k,
                              float* out_scores, int64_t* out_ids, void* stream) {
    if (nq < 0 || n_cand <= 0 || n_rows < 0 || d <= 0 || k <= 0) return RT_ERR_INVALID;
    if (kind != RT_REFINE_F32 && kind != RT_REFINE_F16 && kind != RT_REFINE_BF16 && kind != RT_REFINE_SQ8)
        return RT_ERR_INVALID;
    if (!queries || !cand_ids || !out_scores || !out_ids || (n_rows > 0 && !store)) return RT_ERR_INVALID;
    if (kind == RT_REFINE_SQ8 && (!lo || !step)) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(store)) & 15) return RT_ERR_INVALID;
    if (kind == RT_REFINE_SQ8 && ((reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(step)) & 15))
        return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(cand_ids) | reinterpret_cast<uintptr_t>(out_ids)) & 7) return RT_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(out_scores) & 3) return RT_ERR_INVALID;
    if (n_cand > RT_REFINE_MAX_CAND || k > n_cand || nq > refine::kMaxNq) return RT_ERR_UNSUPPORTED;
    // rows: rt_flatip_topk_online's d / dtype limits; codes: rt_ivf_sq8_topk's
    if (kind == RT_REFINE_SQ8 ? !topk::ivfsq8::d_ok(d) : (d > refine::kMaxD || d % (kind == RT_REFINE_F32 ? 4 : 8)))
        return RT_ERR_UNSUPPORTED;
    if (nq == 0) return RT_OK;
    hipStream_t st = as_stream(stream);
    switch (kind) {
        case RT_REFINE_F32:
            return refine::launch<RT_REFINE_F32>(queries, nq, d, cand_ids, n_cand, store, n_rows, lo, step, k,
                                                 out_scores, out_ids, st);
        case RT_REFINE_F16:
            return refine::launch<RT_REFINE_F16>(queries, nq, d, cand_ids, n_cand, store, n_rows, lo, step, k,
                                                 out_scores, out_ids, st);
        case RT_REFINE_BF16:
            return refine::launch<RT_REFINE_BF16>(queries, nq, d, cand_ids, n_cand, store, n_rows, lo, step, k,
                                                  out_scores, out_ids, st);
        default:
            return refine::launch<RT_REFINE_SQ8>(queries, nq, d, cand_ids, n_cand, store, n_rows, lo, step, k,
                                                 out_scores, out_ids, st);
    }
}
