// rt_tower_infer_f32: the whole eval-mode tower (UserTower.forward,
// src/models/two_tower.py:98-134, as the serving path calls it for one request,
// src/serving/service.py:286-293) for 1..8 rows in ONE launch of ONE workgroup.
//
// Every weight is read once for all rows. Activations stay in LDS (two fp32
// ping-pong buffers [8][512]); the optional id gather is fused into staging
// the input rows. Per layer the loop is GEMV-shaped: a wave owns groups of
// Cols<M> consecutive output columns, its lanes read those rows of W coalesced
// (16-byte loads where k % 4 == 0 and W is 16-byte aligned, dword loads
// otherwise), all loads of a group issued before its first FMA, and FMA them
// against their slice of the M activation rows (ds_read_b128). The M x Cols<M>
// partial sums are folded across the wave by a halving butterfly: log2(M)
// steps that halve the rows a lane carries, then plain xor steps.
//
// Row independence (a contract, tests/test_gpu_tower_infer.py): a row's bits
// do not depend on m or on its slot. A lane's partial sum of (row, column) is
// one sequential fmaf chain over the lane's elements in increasing index; the
// cross-lane sum visits the xor offsets 32, 16, 8, 4, 2, 1 in that order for
// every row in every instantiation (a halving step adds the same two lanes'
// values as the plain step at that offset, and fp32 addition commutes); the
// epilogue and the row normalise are per (row, column) / per row.
//
// No cross-workgroup hand-off, no wait loop: the only synchronisation is
// __syncthreads between layers.
#include "rt_common.h"

namespace rt {
namespace tower {

// 1,024 threads; 512 at M = 8, where 32 accumulators, 32 weight registers and
// the activation reads do not fit 128 VGPRs (the budget of 16 waves on 4 SIMDs)
template <int M>
struct Threads { static constexpr int v = M == 8 ? 512 : 1024; };
// output columns per wave pass (loads in flight: 2 x Cols x 16 B per lane; the
// passes of a layer are a latency chain, so fewer and wider ones where the
// registers allow: 8 columns at M = 1, 4 above)
template <int M>
struct Cols { static constexpr int v = M == 1 ? 8 : 4; };
constexpr int kLd = RT_TOWER_MAX_WIDTH;  // LDS row stride (floats)

template <int M>
struct Log2;
template <> struct Log2<1> { static constexpr int v = 0; };
template <> struct Log2<2> { static constexpr int v = 1; };
template <> struct Log2<4> { static constexpr int v = 2; };
template <> struct Log2<8> { static constexpr int v = 3; };

// Fold acc[M] (one value per row, per lane) across the wave. Afterwards
// acc[0] of lane L holds the wave total of row L >> (6 - log2 M).
// (every index is a compile-time constant: the accumulators stay in registers)
template <int HALF, int OFF, int M>
__device__ __forceinline__ void fold_step(float (&acc)[M], int lane) {
    if constexpr (HALF >= 1) {
        const bool upper = (lane & OFF) != 0;
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
            const float keep = upper ? acc[i + HALF] : acc[i];
            const float send = upper ? acc[i] : acc[i + HALF];
            acc[i] = keep + __shfl_xor(send, OFF, 64);
        }
        fold_step<HALF / 2, OFF / 2>(acc, lane);
    } else if constexpr (OFF >= 1) {
        acc[0] += __shfl_xor(acc[0], OFF, 64);
        fold_step<0, OFF / 2>(acc, lane);
    }
}
template <int M>
__device__ __forceinline__ void fold_rows(float (&acc)[M], int lane) {
    fold_step<M / 2, 32>(acc, lane);
}

template <int M>
__global__ __launch_bounds__(Threads<M>::v) void infer_kernel(const rt_tower_infer_args a) {
    constexpr int kThreads = Threads<M>::v, kWaves = kThreads / RT_WAVE, kCols = Cols<M>::v;
    __shared__ __attribute__((aligned(16))) float buf[2][RT_TOWER_MAX_ROWS * kLd];
    // epilogue parameters of the layer being computed and of the next one, per
    // column: (bias, running_mean, 1/sqrt(running_var + eps), gamma) and beta.
    // Thread j fetches column j of layer l + 1 while layer l computes, so no
    // pass waits for a parameter load.
    __shared__ float4 par[2][RT_TOWER_MAX_WIDTH];
    __shared__ float par_beta[2][RT_TOWER_MAX_WIDTH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m;

    // ---- stage a0 (fused gather); rows m..M-1 and bad ids are zero rows ----
    {
        const int k0 = a.layers[0].k;
        for (int e = tid; e < M * k0; e += kThreads) {
            const int r = e / k0, c = e - r * k0;
            float v = 0.f;
            if (r < m) {
                const int64_t id = a.ids ? a.ids[r] : static_cast<int64_t>(r);
                if (id >= 0 && id < a.src_rows) v = a.src[id * a.ld_src + c];
            }
            buf[0][r * kLd + c] = v;
        }
    }
    auto fetch_params = [&](const rt_tower_layer& P, int j, float4& p, float& beta) {
        p = make_float4(P.bias ? P.bias[j] : 0.f, 0.f, 1.f, 1.f);
        beta = 0.f;
        if (P.bn_gamma) {
            p.y = P.bn_mean[j];
            p.z = 1.f / sqrtf(P.bn_var[j] + P.bn_eps);
            p.w = P.bn_gamma[j];
            beta = P.bn_beta[j];
        }
    };
    if (tid < a.layers[0].n) fetch_params(a.layers[0], tid, par[0][tid], par_beta[0][tid]);
    __syncthreads();

    int cur = 0;
    for (int l = 0; l < a.n_layers; ++l) {
        const rt_tower_layer& L = a.layers[l];
        float4 next_p = make_float4(0.f, 0.f, 0.f, 0.f);
        float next_beta = 0.f;
        const bool fetch_next = l + 1 < a.n_layers && tid < a.layers[l + 1].n;
        if (fetch_next) fetch_params(a.layers[l + 1], tid, next_p, next_beta);
        const float4* pp = par[cur];
        const float* pb = par_beta[cur];
        const int k = L.k, n = L.n;
        const float* __restrict__ W = L.w;
        const float* src = buf[cur];
        float* dst = buf[cur ^ 1];
        const bool vec = (k & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;

        for (int j0 = wave * kCols; j0 < n; j0 += kWaves * kCols) {
            float acc[kCols][M];
#pragma unroll
            for (int u = 0; u < kCols; ++u)
#pragma unroll
                for (int r = 0; r < M; ++r) acc[u][r] = 0.f;
            // a column past n reads column n - 1 (in bounds) and is not written
            const float* wr[kCols];
#pragma unroll
            for (int u = 0; u < kCols; ++u) wr[u] = W + static_cast<size_t>(min(j0 + u, n - 1)) * k;

            if (vec) {
                // k <= 512: at most two 16-byte chunks per lane
                const int nchunk = k >> 2;
                if constexpr (kCols > 4) {
                    // 8 columns: one chunk's weights fill the registers, the second chunk
                    // (k > 256) is a second round of loads
#pragma unroll 1
                    for (int c = lane; c < nchunk; c += 64) {
                        float4 w[kCols];
#pragma unroll
                        for (int u = 0; u < kCols; ++u) w[u] = reinterpret_cast<const float4*>(wr[u])[c];
#pragma unroll
                        for (int r = 0; r < M; ++r) {
                            const float4 x = *reinterpret_cast<const float4*>(src + r * kLd + 4 * c);
#pragma unroll
                            for (int u = 0; u < kCols; ++u) {
                                float s = acc[u][r];
                                s = __builtin_fmaf(w[u].x, x.x, s);
                                s = __builtin_fmaf(w[u].y, x.y, s);
                                s = __builtin_fmaf(w[u].z, x.z, s);
                                s = __builtin_fmaf(w[u].w, x.w, s);
                                acc[u][r] = s;
                            }
                        }
                    }
                } else {
                const int c0 = lane, c1 = lane + 64;
                float4 w0[kCols], w1[kCols];
#pragma unroll
                for (int u = 0; u < kCols; ++u) {
                    w0[u] = c0 < nchunk ? reinterpret_cast<const float4*>(wr[u])[c0] : make_float4(0.f, 0.f, 0.f, 0.f);
                    w1[u] = c1 < nchunk ? reinterpret_cast<const float4*>(wr[u])[c1] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if (c0 < nchunk) {
#pragma unroll
                    for (int r = 0; r < M; ++r) {
                        const float4 x = *reinterpret_cast<const float4*>(src + r * kLd + 4 * c0);
#pragma unroll
                        for (int u = 0; u < kCols; ++u) {
                            float s = acc[u][r];
                            s = __builtin_fmaf(w0[u].x, x.x, s);
                            s = __builtin_fmaf(w0[u].y, x.y, s);
                            s = __builtin_fmaf(w0[u].z, x.z, s);
                            s = __builtin_fmaf(w0[u].w, x.w, s);
                            acc[u][r] = s;
                        }
                    }
                }
                if (c1 < nchunk) {
#pragma unroll
                    for (int r = 0; r < M; ++r) {
                        const float4 x = *reinterpret_cast<const float4*>(src + r * kLd + 4 * c1);
#pragma unroll
                        for (int u = 0; u < kCols; ++u) {
                            float s = acc[u][r];
                            s = __builtin_fmaf(w1[u].x, x.x, s);
                            s = __builtin_fmaf(w1[u].y, x.y, s);
                            s = __builtin_fmaf(w1[u].z, x.z, s);
                            s = __builtin_fmaf(w1[u].w, x.w, s);
                            acc[u][r] = s;
                        }
                    }
                }
                }
            } else {
                // dword loads: lane takes elements lane, lane + 64, ... (covers the k tail)
#pragma unroll 1
                for (int e = lane; e < k; e += 64) {
                    float w[kCols];
#pragma unroll
                    for (int u = 0; u < kCols; ++u) w[u] = wr[u][e];
#pragma unroll
                    for (int r = 0; r < M; ++r) {
                        const float x = src[r * kLd + e];
#pragma unroll
                        for (int u = 0; u < kCols; ++u) acc[u][r] = __builtin_fmaf(w[u], x, acc[u][r]);
                    }
                }
            }

#pragma unroll
            for (int u = 0; u < kCols; ++u) fold_rows<M>(acc[u], lane);

            // epilogue: the lane whose low 6 - log2(M) bits are zero owns row lane >> (6 - log2 M)
            constexpr int kShift = 6 - Log2<M>::v;
            if ((lane & ((1 << kShift) - 1)) == 0) {
                const int r = lane >> kShift;
#pragma unroll
                for (int u = 0; u < kCols; ++u) {
                    const int j = j0 + u;
                    if (j < n) {
                        const float4 p = pp[j];
                        float z = act_eval(L.act, acc[u][0] + p.x);
                        if (L.bn_gamma) z = __builtin_fmaf((z - p.y) * p.z, p.w, pb[j]);
                        dst[r * kLd + j] = z;
                    }
                }
            }
        }
        if (fetch_next) {
            par[cur ^ 1][tid] = next_p;
            par_beta[cur ^ 1][tid] = next_beta;
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- rows out: wave r finishes row r (F.normalize(p=2, eps=1e-12)) ----
    const int n = a.layers[a.n_layers - 1].n;
    const float* z = buf[cur];
    for (int r = wave; r < m; r += kWaves) {
        float scale = 1.f;
        if (a.normalize || a.norms_out) {
            float ss = 0.f;
            for (int e = lane; e < n; e += 64) ss = __builtin_fmaf(z[r * kLd + e], z[r * kLd + e], ss);
            const float norm = sqrtf(wave_sum(ss));
            if (a.norms_out && lane == 0) a.norms_out[r] = norm;
            if (a.normalize) scale = fmaxf(norm, 1e-12f);
        }
        for (int e = lane; e < n; e += 64) a.out[static_cast<size_t>(r) * n + e] = z[r * kLd + e] / scale;
    }
}

}  // namespace tower
}  // namespace rt

using namespace rt;

extern "C" int rt_tower_infer_f32(const rt_tower_infer_args* args, void* stream) {
    if (!args) return RT_ERR_INVALID;
    const rt_tower_infer_args& a = *args;
    if (a.m < 1 || a.m > RT_TOWER_MAX_ROWS || a.n_layers < 1 || a.n_layers > RT_TOWER_MAX_LAYERS)
        return RT_ERR_INVALID;
    if (!a.src || !a.out || a.src_rows < 0 || (!a.ids && a.src_rows < a.m)) return RT_ERR_INVALID;
    for (int l = 0; l < a.n_layers; ++l) {
        const rt_tower_layer& L = a.layers[l];
        if (!L.w || L.k < 1 || L.n < 1 || L.act < RT_ACT_RELU || L.act > RT_ACT_NONE) return RT_ERR_INVALID;
        if (L.bn_gamma && (!L.bn_beta || !L.bn_mean || !L.bn_var)) return RT_ERR_INVALID;
    }
    if (a.ld_src < a.layers[0].k) return RT_ERR_INVALID;
    for (int l = 0; l < a.n_layers; ++l) {
        const rt_tower_layer& L = a.layers[l];
        if (L.k > RT_TOWER_MAX_WIDTH || L.n > RT_TOWER_MAX_WIDTH) return RT_ERR_UNSUPPORTED;
        if (l > 0 && L.k != a.layers[l - 1].n) return RT_ERR_UNSUPPORTED;
    }
    const dim3 grid(1);
    hipStream_t st = as_stream(stream);
    if (a.m == 1)
        hipLaunchKernelGGL(tower::infer_kernel<1>, grid, dim3(tower::Threads<1>::v), 0, st, a);
    else if (a.m == 2)
        hipLaunchKernelGGL(tower::infer_kernel<2>, grid, dim3(tower::Threads<2>::v), 0, st, a);
    else if (a.m <= 4)
        hipLaunchKernelGGL(tower::infer_kernel<4>, grid, dim3(tower::Threads<4>::v), 0, st, a);
    else
        hipLaunchKernelGGL(tower::infer_kernel<8>, grid, dim3(tower::Threads<8>::v), 0, st, a);
    return check_launch("tower_infer_kernel");
}
