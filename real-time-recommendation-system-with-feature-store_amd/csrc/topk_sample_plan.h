// Host arithmetic of the v4 top-K sample (topk_v4.h): which stages a split
// samples, the failure-safe rank of a sampled fraction, and the (stride, rank)
// the planner picks per shape. No device code and no HIP header: topk_api.hip
// includes it, and tests/topk_plan_main.cpp compiles it with plain g++ under
// ASan/UBSan (tests/test_topk_plan_cpu.py).
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>

namespace rt {
namespace topk {
namespace splan {

// mirrors of constants the kernels own; topk_api.hip static_asserts each one
constexpr int kStageRows = 128;  // rows per scan stage (v4::Cfg4::NT)
constexpr int kMaxK = 512;       // largest k of any top-K kernel (topk::kMaxK)
constexpr int kSampleList = 32;  // sampled group maxima kept per query (v4::kSampleList = 2 v4::kList)

// Cap 500 on the expected appends per query, rank / f (round 6; 960 before):
// k = 100 at the C4 shard and the 1M corpus takes stride 32 / rank 15 (~460
// appends) instead of 64 / 11 (~670): the twice denser sample costs less than
// the appends and finish input it saves, 3-7 % at 125K and 2 % at 1M
// (profiles/r06_topk_stride_sweep.txt).
#ifndef RT_TOPK_V4_APPEND_CAP
#define RT_TOPK_V4_APPEND_CAP 500.0
#endif
#ifndef RT_TOPK_V4_MAX_STRIDE
#define RT_TOPK_V4_MAX_STRIDE 64
#endif

// Smallest failure-safe rank: the least r in [1, r_max] with P(Bin(n, f) >= r)
// <= 1e-6 (r > n: probability 0, safe), 0 when none. The binomial tail of
// every r comes from one pass over the pmf (n <= kMaxK terms), summed from the
// top — plan_sample evaluates it for up to 63 strides per plan, on the host
// path of every search call (a log-sum-exp tail per (stride, rank) pair cost
// ~1.7 ms per call at the C4 shapes).
inline int safe_rank(int n, double f, int r_max) {
    static const auto lf = [] {  // log i!
        std::array<double, kMaxK + 2> t{};
        for (int i = 0; i <= kMaxK + 1; ++i) t[i] = std::lgamma(i + 1.0);
        return t;
    }();
    if (n < 0 || n > kMaxK || !(f > 0.0)) return 0;
    if (f >= 1.0) return n + 1 <= r_max ? n + 1 : 0;  // X = n: only r > n is safe
    double tail[kMaxK + 2];
    tail[n + 1] = 0.0;
    const double lf_ = std::log(f), lg = std::log1p(-f);
    for (int i = n; i >= 0; --i) tail[i] = tail[i + 1] + std::exp(lf[n] - lf[i] - lf[n - i] + i * lf_ + (n - i) * lg);
    for (int r = 1; r <= r_max; ++r)
        if (r > n || tail[r] <= 1e-6) return r;
    return 0;
}

// Stages a sample visits, and all stages, of nx rows cut into splits of
// items_per_split rows: every split samples its own stages 0, stride,
// 2·stride, ... (the mode-3 scan; shards of a corpus on several GPUs do the
// same). One split (nx == items_per_split) gives ceil(stages / stride), which
// is also what the joint scan without a presample samples (mode 1: every block
// walks the whole corpus).
struct StageCounts { int64_t sampled, total; };
inline StageCounts sampled_stages(int64_t nx, int64_t items_per_split, int stride) {
    if (nx <= 0 || items_per_split <= 0 || stride < 1) return {0, 0};
    const int64_t nst = (nx + kStageRows - 1) / kStageRows;
    const int64_t sps = (items_per_split + kStageRows - 1) / kStageRows;  // stages per full split
    const int64_t nfull = nst / sps, rem = nst - nfull * sps;
    return {nfull * ((sps + stride - 1) / stride) + (rem + stride - 1) / stride, nst};
}

// (stride, rank) of the sample: the sparsest stride whose smallest safe rank
// keeps the expected candidates per query, rank / f, within
// RT_TOPK_V4_APPEND_CAP; {0, 0} when no stride fits. "Safe": the estimate
// overshoots the k-th score (a rescan) with probability <= 1e-6 — P(>= rank of
// the top k fall in the sample) for a sampled fraction f; the group-maximum
// estimate sits at or below the item rank, so this bounds it. The kernels must
// sample exactly the stages sampled_stages counts: f is the fraction they see.
struct SamplePlan { int stride, rank; };
inline SamplePlan plan_sample(int k, int64_t nx, int64_t items_per_split) {
    for (int st = RT_TOPK_V4_MAX_STRIDE; st >= 2; --st) {
        const StageCounts c = sampled_stages(nx, items_per_split, st);
        if (c.sampled < 4) continue;  // fewer than 32 groups per query in the sample
        const double f = static_cast<double>(c.sampled) / static_cast<double>(c.total);
        const int r = safe_rank(k, f, kSampleList);
        if (r > 0 && r / f <= RT_TOPK_V4_APPEND_CAP) return {st, r};
    }
    return {0, 0};
}

// plan_sample, computed once per (k, rows, rows per split)
inline SamplePlan plan_sample_cached(int k, int64_t nx, int64_t items_per_split) {
    static std::mutex mu;
    static std::map<std::tuple<int, int64_t, int64_t>, SamplePlan> memo;
    const auto key = std::make_tuple(k, nx, items_per_split);
    {
        std::lock_guard<std::mutex> g(mu);
        const auto it = memo.find(key);
        if (it != memo.end()) return it->second;
    }
    const SamplePlan sp = plan_sample(k, nx, items_per_split);
    std::lock_guard<std::mutex> g(mu);
    if (memo.size() > 4096) memo.clear();
    memo[key] = sp;
    return sp;
}

}  // namespace splan
}  // namespace topk
}  // namespace rt
