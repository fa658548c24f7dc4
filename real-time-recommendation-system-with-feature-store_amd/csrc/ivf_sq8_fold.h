// What the two IVF-SQ8 scans share (ivf_sq8.hip, ivf_sq8_batch.hip): the d
// limits, the layout of the folded queries in the workspace and the launch of
// sq8_fold (the kernel itself stays in ivf_sq8.hip).
#pragma once
#include "rt_common.h"

namespace rt {
namespace topk {
namespace ivfsq8 {

constexpr int kMinD = 16, kMaxD = 256;  // whole 16-byte units of codes; the query's LDS

inline bool d_ok(int d) { return d >= kMinD && d <= kMaxD && (d & 15) == 0; }
inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
// floats of one query's fold: qs[d], then base[nprobe] padded to a float4
inline int fold_stride(int d, int nprobe) { return d + ((nprobe + 3) & ~3); }

// one block per query: fold[q] = {qs[q][0..d), base[q][0..nprobe)} (ivf_sq8.hip)
int launch_fold(const float* queries, int64_t nq, int d, const float* lo, const float* step, const float* bias,
                int nprobe, int stride, float* fold, hipStream_t st);

}  // namespace ivfsq8
}  // namespace topk
}  // namespace rt
