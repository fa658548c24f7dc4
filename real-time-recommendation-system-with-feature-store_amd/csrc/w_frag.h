// Fragment-ordered weight images: the fp32 values of a Linear's
// W (forward k-loop) or Wᵀ (dz k-loop) stored in the order the lanes of the
// MFMA k-loops read them, so a wave's W load is 64 consecutive float4 — eight
// whole 128-byte lines — instead of 32 rows x 32 bytes. Host and device share
// the index arithmetic below (tests/w_frag_layout_main.cpp checks it on the CPU).
#ifndef RTREC_W_FRAG_H
#define RTREC_W_FRAG_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_WF_HD __host__ __device__ __forceinline__
#else
#define RT_WF_HD inline
#endif

namespace rt {
namespace wfrag {

RT_WF_HD int pad32(int x) { return (x + 31) / 32 * 32; }

// Forward image of W[n][k]: float4 [T][S][4][64], T = ceil(n/32) column tiles,
// S = pad32(k)/32 k-loop iterations, j = the lane's four loads of an iteration.
RT_WF_HD int fwd_tiles(int n) { return (n + 31) / 32; }
RT_WF_HD int fwd_steps(int k) { return pad32(k) / 32; }
RT_WF_HD int64_t fwd_entries(int n, int k) { return static_cast<int64_t>(fwd_tiles(n)) * fwd_steps(k) * 4 * 64; }
RT_WF_HD int64_t fwd_index(int k, int t, int s, int j, int l) {
    return ((static_cast<int64_t>(t) * fwd_steps(k) + s) * 4 + j) * 64 + l;
}
// entry e holds W[row][col .. col + 3] (zeros where row >= n or col >= k)
RT_WF_HD void fwd_coords(int k, int64_t e, int& row, int& col) {
    const int l = static_cast<int>(e & 63), j = static_cast<int>((e >> 6) & 3);
    const int64_t ts = e >> 8;
    const int S = fwd_steps(k);
    const int s = static_cast<int>(ts % S), t = static_cast<int>(ts / S);
    const int c = l & 31, h = l >> 5;
    row = 32 * t + c;
    col = 32 * s + 16 * (j >> 1) + 8 * h + 4 * (j & 1);
}

// dz image of Wᵀ[k][n] (W is [n][k]): float4 [KT][NS][2][64], KT = ceil(k/32)
// dA column tiles, NS = pad32(n)/16 k-blocks of the reduction over n, j = the
// lane's two loads of a k-block.
RT_WF_HD int dz_tiles(int k) { return (k + 31) / 32; }
RT_WF_HD int dz_steps(int n) { return pad32(n) / 16; }
RT_WF_HD int64_t dz_entries(int n, int k) { return static_cast<int64_t>(dz_tiles(k)) * dz_steps(n) * 2 * 64; }
RT_WF_HD int64_t dz_index(int n, int kt, int sb, int j, int l) {
    return ((static_cast<int64_t>(kt) * dz_steps(n) + sb) * 2 + j) * 64 + l;
}
// entry e holds Wᵀ[trow][tcol .. tcol + 3] = W[tcol + 0..3][trow] (zeros where trow >= k or tcol + q >= n)
RT_WF_HD void dz_coords(int n, int64_t e, int& trow, int& tcol) {
    const int l = static_cast<int>(e & 63), j = static_cast<int>((e >> 6) & 1);
    const int64_t ks = e >> 7;
    const int NS = dz_steps(n);
    const int sb = static_cast<int>(ks % NS), kt = static_cast<int>(ks / NS);
    const int c = l & 31, h = l >> 5;
    trow = 32 * kt + c;
    tcol = 16 * sb + 8 * h + 4 * j;
}

}  // namespace wfrag
}  // namespace rt

#endif  // RTREC_W_FRAG_H
