// rt_mmr_rerank: Maximal Marginal Relevance (Carbonell & Goldstein) over the
// candidates a search returned — the second stage of the reference's request
// path (src/serving/service.py:204-228 retrieves num_recommendations * 10
// candidates and hands them to a ranker), built from what is already resident:
// the candidates' own stored rows.
//
// One workgroup per query, four lanes per candidate (a wave serves 16
// candidates, the block is ceil(n_cand / 16) waves, at most 8). Lane l of a
// candidate owns the 16-byte chunks l, l + 4, l + 8, ... of its row and keeps
// them in REGISTERS for the whole call; the same chunks are written once to LDS
// (storage dtype, at most 130 KiB for 128 fp32 rows of d = 256), which is read
// only as the broadcast of the row chosen in the previous step: every 4-lane
// group reads the same 64 bytes, so the reads are conflict-free.
//
// sim(i, j): each lane runs one sequential fmaf chain over its chunks (chunk
// ascending, element ascending; 16-bit elements widened to fp32), then the four
// partial sums fold in a fixed butterfly (xor 1, xor 2). The order depends on
// (d, dtype) only: no atomics, nothing depends on nq, the block index or
// pos_slot. normalize: the dot times 1/sqrt(|i|^2) times 1/sqrt(|j|^2), the
// squared norms by the same chain and butterfly; a zero row has inverse norm 0.
//
// A step is: update m_i against the row chosen last (one dot), the objective,
// an arg-max inside the wave (shuffles), one LDS slot per wave, ONE barrier,
// and every thread folds the <= 8 slots itself. The slots are double-buffered
// by step parity, so no second barrier is needed.
#include <float.h>

#include "rt_common.h"

namespace rt {
namespace mmr {

constexpr int kMaxCand = RT_MMR_MAX_CAND;
constexpr int kLanes = 4;                              // per candidate
constexpr int kMaxWaves = kMaxCand * kLanes / RT_WAVE;  // 8
constexpr int kMaxD = 256;

// (objective, candidate index); idx < 0 = none. a beats b: larger objective,
// then the lower candidate index.
struct Best {
    float obj;
    int idx;
};
__device__ __forceinline__ bool beats(float oa, int ia, float ob, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return oa > ob || (oa == ob && ia < ib);
}

template <typename T>
struct Chunk;  // 16 bytes of a row, widened on use
template <>
struct Chunk<float> {
    static constexpr int kElems = 4;
    __device__ static __forceinline__ float dot(const uint4& a, const uint4& b, float acc) {
        acc = fmaf(__uint_as_float(a.x), __uint_as_float(b.x), acc);
        acc = fmaf(__uint_as_float(a.y), __uint_as_float(b.y), acc);
        acc = fmaf(__uint_as_float(a.z), __uint_as_float(b.z), acc);
        acc = fmaf(__uint_as_float(a.w), __uint_as_float(b.w), acc);
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
__device__ __forceinline__ float dot16(const uint4& a, const uint4& b, float acc) {
    acc = fmaf(widen_lo<BF>(a.x), widen_lo<BF>(b.x), acc);
    acc = fmaf(widen_hi<BF>(a.x), widen_hi<BF>(b.x), acc);
    acc = fmaf(widen_lo<BF>(a.y), widen_lo<BF>(b.y), acc);
    acc = fmaf(widen_hi<BF>(a.y), widen_hi<BF>(b.y), acc);
    acc = fmaf(widen_lo<BF>(a.z), widen_lo<BF>(b.z), acc);
    acc = fmaf(widen_hi<BF>(a.z), widen_hi<BF>(b.z), acc);
    acc = fmaf(widen_lo<BF>(a.w), widen_lo<BF>(b.w), acc);
    acc = fmaf(widen_hi<BF>(a.w), widen_hi<BF>(b.w), acc);
    return acc;
}
template <>
struct Chunk<__half> {
    static constexpr int kElems = 8;
    __device__ static __forceinline__ float dot(const uint4& a, const uint4& b, float acc) {
        return dot16<false>(a, b, acc);
    }
};
template <>
struct Chunk<__hip_bfloat16> {
    static constexpr int kElems = 8;
    __device__ static __forceinline__ float dot(const uint4& a, const uint4& b, float acc) {
        return dot16<true>(a, b, acc);
    }
};

// the four lanes of a candidate: fixed butterfly, every lane ends with the same bits
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}

// LDS: [n_cand rows of row_stride bytes][inverse norms: n_cand floats][slots: 2 x kMaxWaves Best]
__host__ __device__ inline int row_stride_bytes(int n_chunks) {
    const int b = n_chunks * 16;
    return (b % 128 == 0) ? b + 64 : b;  // neighbouring candidates' b128 writes land on distinct banks
}
__host__ __device__ inline size_t lds_bytes(int n_cand, int n_chunks) {
    return static_cast<size_t>(n_cand) * row_stride_bytes(n_chunks) + static_cast<size_t>(n_cand) * 4 +
           2 * kMaxWaves * sizeof(Best);
}

template <typename T>
__global__ __launch_bounds__(kMaxCand* kLanes) void mmr_rerank_kernel(
    const float* __restrict__ cand_scores, const int64_t* __restrict__ cand_ids, int n_cand,
    const uint4* __restrict__ rows, int64_t n_rows, int n_chunks, const int32_t* __restrict__ pos_slot,
    int64_t n_pos, const float* __restrict__ lambda, int normalize, int k, float* __restrict__ out_scores,
    int64_t* __restrict__ out_ids) {
    constexpr int kMaxJ = kMaxD / Chunk<T>::kElems / kLanes;  // chunks a lane may own: 16 (fp32), 8 (16-bit)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int stride = row_stride_bytes(n_chunks);
    float* const inv_s = reinterpret_cast<float*>(smem + static_cast<size_t>(n_cand) * stride);
    Best* const slots = reinterpret_cast<Best*>(inv_s + n_cand);  // 4-byte aligned, as Best is

    const int64_t q = blockIdx.x;
    const int i = threadIdx.x >> 2, l = threadIdx.x & 3;  // candidate, lane of the candidate
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;

    float lam = lambda[q];
    lam = lam < 0.f ? 0.f : (lam > 1.f ? 1.f : lam);  // a NaN stays a NaN: nothing is selected wrongly, only arbitrarily
    const float oml = 1.f - lam;

    // ---- my candidate: id -> slot, present or absent ----
    float score = -FLT_MAX;
    int64_t id = -1;
    int64_t slot = -1;
    if (i < n_cand) {
        score = cand_scores[q * n_cand + i];
        id = cand_ids[q * n_cand + i];
        if (id >= 0 && id < n_pos) slot = pos_slot ? static_cast<int64_t>(pos_slot[id]) : id;
    }
    const bool present = slot >= 0 && slot < n_rows;  // an absent candidate's row is never read

    // ---- my chunks: registers, and LDS for whoever gets to read this row as the chosen one ----
    uint4 mine[kMaxJ];
    float nrm = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxJ; ++j) {
        const int c = l + kLanes * j;
        mine[j] = make_uint4(0u, 0u, 0u, 0u);
        if (present && c < n_chunks) {
            mine[j] = rows[slot * n_chunks + c];
            *reinterpret_cast<uint4*>(smem + static_cast<size_t>(i) * stride + c * 16) = mine[j];
            nrm = Chunk<T>::dot(mine[j], mine[j], nrm);
        }
    }
    float inv = 1.f;
    if (normalize) {  // block-uniform
        nrm = group_sum(nrm);
        inv = nrm > 0.f ? 1.f / sqrtf(nrm) : 0.f;
        if (present && l == 0) inv_s[i] = inv;
    }
    __syncthreads();

    bool open = present;  // present and not yet chosen
    float m = 0.f;        // max similarity to the chosen ones; 0 while none is chosen
    int prev = -1;
    int t = 0;
    for (; t < k; ++t) {
        if (prev >= 0) {  // block-uniform
            const unsigned char* const pr = smem + static_cast<size_t>(prev) * stride;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxJ; ++j) {
                const int c = l + kLanes * j;
                if (c < n_chunks) acc = Chunk<T>::dot(mine[j], *reinterpret_cast<const uint4*>(pr + c * 16), acc);
            }
            float sim = group_sum(acc);
            if (normalize) sim *= inv * inv_s[prev];
            m = (t == 1) ? sim : fmaxf(m, sim);
        }
        float obj = fmaf(lam, score, -(oml * m));
        int idx = open ? i : -1;
        // arg-max of the wave: the four lanes of a candidate agree, so offsets 4..32 suffice
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) {
            const float oo = __shfl_xor(obj, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (beats(oo, oi, obj, idx)) {
                obj = oo;
                idx = oi;
            }
        }
        Best* const sl = slots + (t & 1) * kMaxWaves;
        if ((threadIdx.x & 63) == 0) sl[wave] = Best{obj, idx};
        __syncthreads();
        Best b = sl[0];
        for (int w = 1; w < n_waves; ++w) {
            const Best o = sl[w];
            if (beats(o.obj, o.idx, b.obj, b.idx)) b = o;
        }
        if (b.idx < 0) break;  // block-uniform: nothing left to choose
        if (b.idx == i) {
            open = false;
            if (l == 0) {
                out_scores[q * k + t] = score;
                out_ids[q * k + t] = id;
            }
        }
        prev = b.idx;
    }
    for (int p = t + static_cast<int>(threadIdx.x); p < k; p += blockDim.x) {
        out_scores[q * k + p] = -FLT_MAX;
        out_ids[q * k + p] = -1;
    }
}

}  // namespace mmr
}  // namespace rt

using namespace rt;

namespace {
// allow > 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU); set once per kernel
template <auto Kernel>
void allow_lds(size_t bytes) {
    static size_t set = 0;
    if (bytes > set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(bytes));
        set = bytes;
    }
}

template <typename T>
int launch_mmr(const float* cand_scores, const int64_t* cand_ids, int64_t nq, int n_cand, const void* rows,
               int64_t n_rows, int d, const int32_t* pos_slot, int64_t n_pos, const float* lambda, int normalize,
               int k, float* out_scores, int64_t* out_ids, hipStream_t st) {
    const int n_chunks = d / mmr::Chunk<T>::kElems;
    const size_t lds = mmr::lds_bytes(n_cand, n_chunks);
    allow_lds<mmr::mmr_rerank_kernel<T>>(lds);
    const int threads = (n_cand * mmr::kLanes + RT_WAVE - 1) / RT_WAVE * RT_WAVE;
    constexpr int64_t kGrid = 1ll << 30;
    for (int64_t q0 = 0; q0 < nq; q0 += kGrid) {
        const int64_t n = (nq - q0) < kGrid ? (nq - q0) : kGrid;
        hipLaunchKernelGGL(mmr::mmr_rerank_kernel<T>, dim3(static_cast<unsigned>(n)), dim3(threads), lds, st,
                           cand_scores + q0 * n_cand, cand_ids + q0 * n_cand, n_cand,
                           reinterpret_cast<const uint4*>(rows), n_rows, n_chunks, pos_slot, n_pos, lambda + q0,
                           normalize, k, out_scores + q0 * k, out_ids + q0 * k);
        const int rc = check_launch("mmr_rerank_kernel");
        if (rc) return rc;
    }
    return RT_OK;
}

// bytes of an [nq, per_row] array, saturating: any nq a caller can give is answered without overflow
uint64_t array_bytes(int64_t nq, int per_row, int elem) {
    const uint64_t row = static_cast<uint64_t>(per_row) * static_cast<uint64_t>(elem);
    const uint64_t cap = UINT64_MAX / 4;
    return static_cast<uint64_t>(nq) > cap / row ? cap : static_cast<uint64_t>(nq) * row;
}
bool overlaps(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    const uint64_t ea = pa + a_bytes < pa ? UINT64_MAX : pa + a_bytes, eb = pb + b_bytes < pb ? UINT64_MAX : pb + b_bytes;
    return pa < eb && pb < ea;
}
}  // namespace

extern "C" int rt_mmr_rerank(const float* cand_scores, const int64_t* cand_ids, int64_t nq, int n_cand,
                             const void* rows, int64_t n_rows, int d, int dtype, const int32_t* pos_slot,
                             int64_t n_pos, const float* lambda, int normalize, int k, float* out_scores,
                             int64_t* out_ids, void* stream) {
    if (nq < 0 || n_cand <= 0 || n_rows < 0 || n_pos < 0 || d <= 0 || k <= 0) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!cand_scores || !cand_ids || !lambda || !out_scores || !out_ids || (n_rows > 0 && !rows))
        return RT_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(rows) & 15) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(cand_scores) | reinterpret_cast<uintptr_t>(lambda) |
         reinterpret_cast<uintptr_t>(out_scores) | reinterpret_cast<uintptr_t>(pos_slot)) & 3)
        return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(cand_ids) | reinterpret_cast<uintptr_t>(out_ids)) & 7) return RT_ERR_INVALID;
    if (n_cand > RT_MMR_MAX_CAND || k > n_cand) return RT_ERR_UNSUPPORTED;
    if (d > mmr::kMaxD || d % (dtype == RT_F32 ? 4 : 8) != 0) return RT_ERR_UNSUPPORTED;
    if (n_pos >= 0x7FFFFFFFll) return RT_ERR_UNSUPPORTED;  // positions are int32
    const uint64_t in_s = array_bytes(nq, n_cand, 4), in_i = array_bytes(nq, n_cand, 8),
                   out_s = array_bytes(nq, k, 4), out_i = array_bytes(nq, k, 8);
    if (overlaps(out_scores, out_s, cand_scores, in_s) || overlaps(out_scores, out_s, cand_ids, in_i) ||
        overlaps(out_ids, out_i, cand_scores, in_s) || overlaps(out_ids, out_i, cand_ids, in_i) ||
        overlaps(out_scores, out_s, out_ids, out_i))
        return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    hipStream_t st = as_stream(stream);
    switch (dtype) {
        case RT_F32:
            return launch_mmr<float>(cand_scores, cand_ids, nq, n_cand, rows, n_rows, d, pos_slot, n_pos, lambda,
                                     normalize, k, out_scores, out_ids, st);
        case RT_F16:
            return launch_mmr<__half>(cand_scores, cand_ids, nq, n_cand, rows, n_rows, d, pos_slot, n_pos, lambda,
                                      normalize, k, out_scores, out_ids, st);
        default:
            return launch_mmr<__hip_bfloat16>(cand_scores, cand_ids, nq, n_cand, rows, n_rows, d, pos_slot, n_pos,
                                              lambda, normalize, k, out_scores, out_ids, st);
    }
}
