// Beyond-accuracy list metrics (src/evaluation/metrics.py:402-478): intra-list
// diversity (mean pairwise cosine distance of a list's first k items) and
// novelty (mean self-information of the recommended items), per ranking row on
// the device, for every k of one call in a single pass over the row.
//
// Diversity never forms the K×K similarity matrix: with ê = e / (‖e‖ + 1e-8),
//   Σ_{i<j} ê_i·ê_j = (‖Σ ê_i‖² − Σ ‖ê_i‖²) / 2
// so a row keeps the running vector s = Σ ê_i and the scalar q = Σ ‖ê_i‖² in
// rank order and emits 1 − (‖s‖² − q) / (n(n−1)) at every k boundary and at the
// end of the list: O(K·d) per row. All arithmetic is fp64 on the stored values.
//
// A row gather from the embedding table, latency-bound: one wave per row, the
// wave split into groups of G lanes that each own one list entry (G·16 B covers
// an embedding row; G = 64 and several vectors per lane for long rows), and the
// loads of kU entries per group (8·64/G entries per wave) are issued before the
// first reduction. No floating-point atomics: per-row results are plain stores,
// the summary is a fixed-order reduction.
#include "rt_common.h"

namespace rt {
namespace listm {

constexpr int kMaxK = RT_METRICS_MAX_K;
constexpr int kU = 8;  // list entries whose row loads a group issues back to back

struct KList {
    int v[kMaxK];
    int n;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int DT>
__device__ __forceinline__ double elem16(uint32_t bits) {
    return static_cast<double>(DT == RT_F16 ? bits_f16_to_f32(static_cast<uint16_t>(bits))
                                            : bits_bf16_to_f32(static_cast<uint16_t>(bits)));
}

// sum over the lanes of one group (G a power of two): xor offsets below G
__device__ __forceinline__ double group_sum(double v, int G) {
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over the groups of the wave, lane by lane: xor offsets G and above
__device__ __forceinline__ double across_groups(double v, int G) {
    for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row r. DT: element type of the table. VEC: 16-byte units (4 fp32
// or 8 16-bit elements), else one element per unit. VPL: units per lane and
// entry. A row of the table has `units` units; lane gl of a group reads units
// gl, gl + G, … (< units).
template <int DT, bool VEC, int VPL>
__global__ __launch_bounds__(256) void list_metrics_kernel(
    const int64_t* __restrict__ preds, int64_t n_rows, int list_len, const char* __restrict__ emb, int64_t n_emb,
    int units, int G, int64_t ld_bytes, const double* __restrict__ info, int64_t n_info, double default_info,
    KList K, double* __restrict__ div, int32_t* __restrict__ div_valid, double* __restrict__ nov_sum,
    int32_t* __restrict__ nov_cnt, int32_t* __restrict__ oob) {
    constexpr int NE = VEC ? (DT == RT_F32 ? 4 : 8) : 1;  // elements per unit
    constexpr int W = VEC ? 4 : 1;                        // 32-bit words per unit
    __shared__ int64_t ids_sm[4][64];
    __shared__ int ksm[kMaxK];
#pragma unroll
    for (int i = 0; i < kMaxK; ++i)
        if (threadIdx.x == i) ksm[i] = K.v[i];
    __syncthreads();
    const int wv = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + wv;
    if (r >= n_rows) return;  // wave-uniform, no block barriers below
    const int nk = K.n;
    const int E = 64 / G;  // entries a wave handles side by side
    const int gl = lane & (G - 1);
    const int g = lane / G;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));  // lanes below this one

    double s[VPL][NE];  // this group's share of Σ ê, this lane's elements
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int c = 0; c < NE; ++c) s[v][c] = 0.0;
    double q = 0.0;  // this group's share of Σ ‖ê‖² (the same in each of its lanes)
    int dbase = 0;   // diversity: entries of the list before this chunk
    int ki = 0;      // next k boundary to emit
    double band[kMaxK];  // novelty: Σ info over ranks [k_{i-1}, k_i)
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) band[i] = 0.0;
    int nbase = 0;  // novelty: present entries before this chunk

    // diversity of the first n entries from the running sums
    auto diversity = [&](int n) -> double {
        double ns = 0.0;
#pragma unroll
        for (int v = 0; v < VPL; ++v)
#pragma unroll
            for (int c = 0; c < NE; ++c) {
                const double t = across_groups(s[v][c], G);
                ns += t * t;
            }
        ns = group_sum(ns, G);
        const double qt = across_groups(q, G);
        const double nn = static_cast<double>(n);
        return 1.0 - (ns - qt) / (nn * (nn - 1.0));
    };

    const int64_t* row = preds + r * static_cast<int64_t>(list_len);
    for (int j0 = 0; j0 < list_len; j0 += 64) {
        const int j = j0 + lane;
        const int64_t id = j < list_len ? row[j] : -1;
        const bool present = id >= 0;  // -1 pads a ragged list (the rule of rt_rank_metrics)

        if (info) {
            const uint64_t pm = __ballot(present);
            const int cnt = __popcll(pm);
            const int rank = nbase + __popcll(pm & lt);
            double val = 0.0;
            if (present) val = id < n_info ? info[id] : default_info;
#pragma unroll
            for (int i = 0; i < kMaxK; ++i) {
                if (i < nk) {
                    const int lo = i ? K.v[i - 1] : 0, hi = K.v[i];
                    if (lo < nbase + cnt && hi > nbase)  // the band meets this chunk (wave-uniform)
                        band[i] += wave_sum((present && rank >= lo && rank < hi) ? val : 0.0);
                }
            }
            nbase += cnt;
        }

        if (emb) {
            const bool inb = present && id < n_emb;  // bounds check before any row read
            if (present && !inb && oob) atomicAdd(oob, 1);
            const uint64_t km = __ballot(inb);
            const int cnt = __popcll(km);
            if (inb) ids_sm[wv][__popcll(km & lt)] = id;  // the chunk's list, compacted in rank order
            wave_lds_sync();
            int pos = 0;
            while (pos < cnt) {
                const int next_b = ki < nk ? ksm[ki] : 0x7FFFFFFF;
                const int room = next_b - dbase;  // > pos: boundaries strictly ascend
                const int seg_end = cnt < room ? cnt : room;
                for (int e0 = pos; e0 < seg_end; e0 += E * kU) {
                    uint32_t raw[kU][VPL][W];
#pragma unroll
                    for (int u = 0; u < kU; ++u) {
                        const int e = e0 + u * E + g;
                        const bool has = e < seg_end;
                        const char* rp = emb;
                        if (has) rp += ids_sm[wv][e] * ld_bytes;
#pragma unroll
                        for (int v = 0; v < VPL; ++v) {
                            const int unit = v * G + gl;
                            const bool ld = has && unit < units;
                            if constexpr (VEC) {
                                u32x4 x = {0u, 0u, 0u, 0u};
                                if (ld) x = reinterpret_cast<const u32x4*>(rp)[unit];
                                raw[u][v][0] = x.x;
                                raw[u][v][1] = x.y;
                                raw[u][v][2] = x.z;
                                raw[u][v][3] = x.w;
                            } else if constexpr (DT == RT_F32) {
                                raw[u][v][0] = ld ? reinterpret_cast<const uint32_t*>(rp)[unit] : 0u;
                            } else {
                                raw[u][v][0] = ld ? static_cast<uint32_t>(reinterpret_cast<const uint16_t*>(rp)[unit]) : 0u;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u) {
                        double x[VPL][NE];
                        double n2 = 0.0;
#pragma unroll
                        for (int v = 0; v < VPL; ++v) {
                            if constexpr (DT == RT_F32) {
#pragma unroll
                                for (int c = 0; c < NE; ++c) x[v][c] = static_cast<double>(__uint_as_float(raw[u][v][c]));
                            } else if constexpr (VEC) {
#pragma unroll
                                for (int c = 0; c < W; ++c) {
                                    x[v][2 * c] = elem16<DT>(raw[u][v][c] & 0xFFFFu);
                                    x[v][2 * c + 1] = elem16<DT>(raw[u][v][c] >> 16);
                                }
                            } else {
                                x[v][0] = elem16<DT>(raw[u][v][0]);
                            }
#pragma unroll
                            for (int c = 0; c < NE; ++c) n2 += x[v][c] * x[v][c];
                        }
                        n2 = group_sum(n2, G);  // every lane takes part: absent entries carry zeros
                        const double inv = 1.0 / (sqrt(n2) + 1e-8);  // eps on the norm, as the reference
#pragma unroll
                        for (int v = 0; v < VPL; ++v)
#pragma unroll
                            for (int c = 0; c < NE; ++c) s[v][c] += x[v][c] * inv;
                        q += n2 * inv * inv;
                    }
                }
                if (dbase + seg_end == next_b) {  // the list reached k_ki entries
                    const double dv = diversity(next_b);
                    if (lane == 0) {
                        div[r * nk + ki] = next_b >= 2 ? dv : 0.0;
                        div_valid[r * nk + ki] = next_b >= 2 ? 1 : 0;
                    }
                    ++ki;
                }
                pos = seg_end;
            }
            dbase += cnt;
        }
    }

    if (emb && ki < nk) {  // lists shorter than k: every remaining k sees the whole list
        const bool ok = dbase >= 2;
        const double dv = ok ? diversity(dbase) : 0.0;
        if (lane == 0)
            for (int i = ki; i < nk; ++i) {
                div[r * nk + i] = dv;
                div_valid[r * nk + i] = ok ? 1 : 0;
            }
    }
    if (info && lane == 0) {
        double run = 0.0;
#pragma unroll
        for (int i = 0; i < kMaxK; ++i) {
            if (i < nk) {
                run += band[i];
                nov_sum[r * nk + i] = run;
                nov_cnt[r * nk + i] = nbase < K.v[i] ? nbase : K.v[i];
            }
        }
    }
}

// Per k, in a fixed order (deterministic): thread t sums rows t, t+256, …
// sequentially, then a fixed LDS tree. out fp64 [4][n_k]: diversity mean over
// the valid rows, number of valid rows, Σ nov_sum / Σ nov_cnt, Σ nov_cnt.
__global__ __launch_bounds__(256) void list_metrics_reduce_kernel(const double* __restrict__ div,
                                                                  const int32_t* __restrict__ div_valid,
                                                                  const double* __restrict__ nov_sum,
                                                                  const int32_t* __restrict__ nov_cnt,
                                                                  int64_t n_rows, int nk, double* __restrict__ out) {
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    for (int i = 0; i < nk; ++i) {
        double ds = 0.0, ns = 0.0;
        int64_t dn = 0, nn = 0;
#pragma unroll 4
        for (int64_t r = t; r < n_rows; r += 256) {
            const int64_t o = r * nk + i;
            if (div && div_valid[o]) { ds += div[o]; ++dn; }
            if (nov_sum) { ns += nov_sum[o]; nn += nov_cnt[o]; }
        }
        red[0][t] = ds;
        red[1][t] = static_cast<double>(dn);
        red[2][t] = ns;
        red[3][t] = static_cast<double>(nn);
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (t < st) {
#pragma unroll
                for (int c = 0; c < 4; ++c) red[c][t] += red[c][t + st];
            }
            __syncthreads();
        }
        if (t == 0) {
            out[i] = red[1][0] > 0.0 ? red[0][0] / red[1][0] : 0.0;
            out[nk + i] = red[1][0];
            out[2 * nk + i] = red[3][0] > 0.0 ? red[2][0] / red[3][0] : 0.0;
            out[3 * nk + i] = red[3][0];
        }
        __syncthreads();
    }
}

inline int pow2_ceil(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace listm
}  // namespace rt

using namespace rt;

#define RT_LISTM_LAUNCH(DT, VEC, VPL)                                                                             \
    hipLaunchKernelGGL((listm::list_metrics_kernel<DT, VEC, VPL>), dim3(static_cast<unsigned>(blocks)), dim3(256), \
                       0, as_stream(stream), preds, n_rows, list_len, static_cast<const char*>(emb), n_emb, units, \
                       G, ld_bytes, info, n_info, default_info, K, div, div_valid, nov_sum, nov_cnt, oob_count)

extern "C" int rt_list_metrics(const int64_t* preds, int64_t n_rows, int list_len, const void* emb, int emb_dtype,
                               int64_t n_emb, int d, int64_t ld_emb, const double* info, int64_t n_info,
                               double default_info, const int32_t* k_values, int n_k, double* div,
                               int32_t* div_valid, double* nov_sum, int32_t* nov_cnt, int32_t* oob_count,
                               void* stream) {
    if (n_rows < 0 || list_len < 0 || n_k < 1 || n_k > listm::kMaxK || !k_values) return RT_ERR_INVALID;
    listm::KList K{};
    K.n = n_k;
    for (int i = 0; i < n_k; ++i) {  // host array, ascending positive
        if (k_values[i] <= 0 || (i > 0 && k_values[i] <= k_values[i - 1])) return RT_ERR_INVALID;
        K.v[i] = k_values[i];
    }
    if (!emb && !info) return RT_ERR_INVALID;  // nothing to compute
    if (emb) {
        if (emb_dtype != RT_F32 && emb_dtype != RT_F16 && emb_dtype != RT_BF16) return RT_ERR_INVALID;
        if (d < 1 || n_emb < 0 || ld_emb < d || !div || !div_valid) return RT_ERR_INVALID;
        if (d > 1024 || (emb_dtype != RT_F32 && (d & 7))) return RT_ERR_UNSUPPORTED;
    }
    if (info && (n_info < 0 || !nov_sum || !nov_cnt)) return RT_ERR_INVALID;
    if (list_len > 0 && !preds) return RT_ERR_INVALID;
    if (n_rows == 0) return RT_OK;
    const int64_t blocks = (n_rows + 3) / 4;
    if (blocks > (1ll << 31) - 1) return RT_ERR_UNSUPPORTED;

    int units = 1, G = 64;
    int64_t ld_bytes = 0;
    if (!emb) {
        RT_LISTM_LAUNCH(RT_F32, false, 1);
        return check_launch("list_metrics_kernel");
    }
    const int es = emb_dtype == RT_F32 ? 4 : 2;
    ld_bytes = ld_emb * es;
    const uintptr_t base = reinterpret_cast<uintptr_t>(emb);
    if (base & (es - 1)) return RT_ERR_INVALID;
    const bool vec = ((static_cast<int64_t>(d) * es) & 15) == 0 && (ld_bytes & 15) == 0 && (base & 15) == 0;
    if (vec) {
        units = d * es / 16;
        G = listm::pow2_ceil(units < 64 ? units : 64);
        const int vpl = (units + 63) / 64;  // fp32: up to 4; 16-bit: up to 2
        if (emb_dtype == RT_F32) {
            if (vpl == 1) RT_LISTM_LAUNCH(RT_F32, true, 1);
            else if (vpl == 2) RT_LISTM_LAUNCH(RT_F32, true, 2);
            else RT_LISTM_LAUNCH(RT_F32, true, 4);
        } else if (emb_dtype == RT_F16) {
            if (vpl == 1) RT_LISTM_LAUNCH(RT_F16, true, 1);
            else RT_LISTM_LAUNCH(RT_F16, true, 2);
        } else {
            if (vpl == 1) RT_LISTM_LAUNCH(RT_BF16, true, 1);
            else RT_LISTM_LAUNCH(RT_BF16, true, 2);
        }
    } else {  // scalar path: one element per unit, the whole wave on one entry
        units = d;
        G = 64;
        const int cpl = (d + 63) / 64;
        if (emb_dtype == RT_F32) {
            if (cpl == 1) RT_LISTM_LAUNCH(RT_F32, false, 1);
            else if (cpl <= 4) RT_LISTM_LAUNCH(RT_F32, false, 4);
            else RT_LISTM_LAUNCH(RT_F32, false, 16);
        } else if (emb_dtype == RT_F16) {
            RT_LISTM_LAUNCH(RT_F16, false, 16);
        } else {
            RT_LISTM_LAUNCH(RT_BF16, false, 16);
        }
    }
    return check_launch("list_metrics_kernel");
}

extern "C" int rt_list_metrics_reduce(const double* div, const int32_t* div_valid, const double* nov_sum,
                                      const int32_t* nov_cnt, int64_t n_rows, int n_k, double* out, void* stream) {
    if (n_rows < 0 || n_k < 1 || n_k > listm::kMaxK || !out) return RT_ERR_INVALID;
    if ((div != nullptr) != (div_valid != nullptr) || (nov_sum != nullptr) != (nov_cnt != nullptr)) return RT_ERR_INVALID;
    if (n_rows > 0 && !div && !nov_sum) return RT_ERR_INVALID;
    hipLaunchKernelGGL(listm::list_metrics_reduce_kernel, dim3(1), dim3(256), 0, as_stream(stream), div, div_valid,
                       nov_sum, nov_cnt, n_rows, n_k, out);
    return check_launch("list_metrics_reduce_kernel");
}
