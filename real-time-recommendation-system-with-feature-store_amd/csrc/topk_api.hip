// C ABI for the Flat-IP top-K (rt_flatip_topk) and the candidate-list merge
// (rt_topk_merge, used for split corpora and for the multi-GPU merge of
// per-shard top-K lists after an RCCL all-gather).
#include "topk_impl.h"
#include "topk_sample_plan.h"

namespace rt {
namespace topk {

// ---- merge [n_lists][nq][k_in] → [nq][k_out], one wave per query ----
// Candidates stream through a per-wave LDS buffer of N entries: the first
// k_out slots keep the running best, the rest take new candidates, then sort.
// ids are carried as uint32 (0 <= id < 2^32-1).
constexpr int kMergeN = 1024;

// Small merges (n_lists·k_in <= 64·E, k_out <= 64·E; C3's 9 lists of 10, two
// shards of 100) sort in registers: E candidates per lane, one register
// bitonic sort, no LDS (the LDS form below costs ~16 µs at C3).
template <int E>
__global__ __launch_bounds__(256) void topk_merge_regs_kernel(const float* __restrict__ s_in,
                                                              const int64_t* __restrict__ i_in, int64_t nq,
                                                              int n_lists, int k_in, int k_out,
                                                              float* __restrict__ s_out,
                                                              int64_t* __restrict__ i_out) {
    const int lane = threadIdx.x & 63;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int total = n_lists * k_in;
    float sv[E];
    uint32_t iv[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int e = lane * E + j;
        sv[j] = -INFINITY;
        iv[j] = kEmptyId;
        if (e < total) {
            const int l = e / k_in, c = e - l * k_in;
            const int64_t off = (static_cast<int64_t>(l) * nq + q) * k_in + c;
            const int64_t id = i_in[off];
            if (id >= 0) { sv[j] = s_in[off]; iv[j] = static_cast<uint32_t>(id); }
        }
    }
    wave_sort_regs<E>(sv, iv);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int e = lane * E + j;
        if (e < k_out) {
            const bool ok = iv[j] != kEmptyId;
            s_out[q * k_out + e] = ok ? sv[j] : -FLT_MAX;
            i_out[q * k_out + e] = ok ? static_cast<int64_t>(iv[j]) : -1;
        }
    }
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ s_in,
                                                         const int64_t* __restrict__ i_in, int64_t nq,
                                                         int n_lists, int k_in, int k_out,
                                                         float* __restrict__ s_out,
                                                         int64_t* __restrict__ i_out) {
    __shared__ Cand buf[4][kMergeN];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 4 + w;
    if (q >= nq) return;
    Cand* b = buf[w];
    const int64_t total = static_cast<int64_t>(n_lists) * k_in;
    int want = total < kMergeN ? static_cast<int>(total) : kMergeN;
    if (want < k_out + 64) want = k_out + 64;  // room for new candidates each round
    int n = next_pow2(want);
    if (n > kMergeN) n = kMergeN;
    int kept = 0;
    int64_t next = 0;
    for (;;) {
        for (int e = kept + lane; e < n; e += 64) {
            const int64_t src = next + (e - kept);
            Cand c{-INFINITY, kEmptyId};
            if (src < total) {
                const int l = static_cast<int>(src / k_in);
                const int j = static_cast<int>(src - static_cast<int64_t>(l) * k_in);
                const int64_t off = (static_cast<int64_t>(l) * nq + q) * k_in + j;
                const int64_t id = i_in[off];
                if (id >= 0) c = Cand{s_in[off], static_cast<uint32_t>(id)};
            }
            b[e] = c;
        }
        next += n - kept;
        wave_lds_sync();
        wave_sort_lds(b, n);
        kept = k_out;
        if (next >= total) break;
    }
    for (int e = lane; e < k_out; e += 64) {
        const Cand c = b[e];
        const bool ok = c.i != kEmptyId;
        s_out[q * k_out + e] = ok ? c.s : -FLT_MAX;
        i_out[q * k_out + e] = ok ? static_cast<int64_t>(c.i) : -1;
    }
}

// Merges of <= 1024 candidates into <= 128 (the owner merge of the multi-GPU
// top-K: N lists of k = 100; C3's split lists): the v4 finish's register
// select. Each lane holds 16 candidates as composite keys (score key << 32 |
// ~id), a radix select starting below the keys' shared prefix cuts them to
// <= 128, and the unrolled 128-entry sort writes the k_out best — instead of a
// 512/1024-entry LDS bitonic sort (176 us for 8 lists x 8,192 queries).
__global__ __launch_bounds__(256) void topk_merge_select_kernel(const float* __restrict__ s_in,
                                                                const int64_t* __restrict__ i_in, int64_t nq,
                                                                int n_lists, int k_in, int k_out,
                                                                float* __restrict__ s_out,
                                                                int64_t* __restrict__ i_out) {
    constexpr int R = v4::kFinishRegs;
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[4][256];
    __shared__ __attribute__((aligned(16))) Cand keep_all[4][v4::kFinishCap];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 4 + w;
    if (q >= nq) return;
    const int total = n_lists * k_in;  // <= 64 R (host-checked)
    uint64_t key[R];
    uint32_t vmask = 0u;
    // slot e of this lane: flat entry f = 64 e + lane = (list l, position j)
    int l = lane / k_in, j = lane - (lane / k_in) * k_in;
#pragma unroll
    for (int e = 0; e < R; ++e) {
        key[e] = 0ull;
        if (e * 64 + lane < total) {
            const int64_t off = (static_cast<int64_t>(l) * nq + q) * k_in + j;
            const int64_t id = i_in[off];
            if (id >= 0) {
                key[e] = v4::ckey(Cand{s_in[off], static_cast<uint32_t>(id)});
                vmask |= 1u << e;
            }
        }
        j += 64;
        while (j >= k_in) { j -= k_in; ++l; }
    }
    uint64_t mx = 0ull, mn = ~0ull;
    int nv = 0;
#pragma unroll
    for (int e = 0; e < R; ++e)
        if ((vmask >> e) & 1u) {
            mx = key[e] > mx ? key[e] : mx;
            mn = key[e] < mn ? key[e] : mn;
            ++nv;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t a = __shfl_xor(mx, o, 64), b = __shfl_xor(mn, o, 64);
        mx = a > mx ? a : mx;
        mn = b < mn ? b : mn;
        nv += __shfl_xor(nv, o, 64);
    }
    Cand* keep = keep_all[w];
    int m = 0;
    if (nv > 0) {
        int shift = 64 - (mx == mn ? 64 : __builtin_clzll(mx ^ mn));  // bits below the shared prefix
        if (shift < 8) shift = 8;
        uint64_t prefix = mx & v4::prefix_mask(shift);
        int kept = nv;
        auto eachr = [&](auto&& fn) {
#pragma unroll
            for (int e = 0; e < R; ++e)
                if ((vmask >> e) & 1u) fn(key[e]);
        };
        if (nv > v4::kFinishCap) v4::radix_prefix(eachr, k_out, v4::kFinishCap, hist_all[w], prefix, shift, kept);
        const uint64_t pmask = v4::prefix_mask(shift);
        // entries above the boundary bucket first, then the bucket up to the
        // cap: a bucket still over the cap after all 64 bits holds copies of one
        // (score, id) — the same entry listed twice — so any of them may go
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int e = 0; e < R; ++e) {
                const uint64_t kb = key[e] & pmask;
                const bool take = ((vmask >> e) & 1u) && (pass == 0 ? kb > prefix : kb == prefix);
                const uint64_t bm = __ballot(take);
                const int pos = m + ballot_rank(bm);
                if (take && pos < v4::kFinishCap)
                    keep[pos] = Cand{v2::okey_inv(static_cast<uint32_t>(key[e] >> 32)), ~static_cast<uint32_t>(key[e])};
                m += __popcll(bm);
            }
        }
        if (m > v4::kFinishCap) m = v4::kFinishCap;
    }
    wave_lds_sync();
    v4::finish_sort<2>(keep, m, k_out, s_out + q * k_out, i_out + q * k_out, 0);
}

int launch_merge(const float* s, const int64_t* ids, int64_t nq, int n_lists, int k_in, int k_out,
                 float* os, int64_t* oi, hipStream_t st) {
    if (k_out + 64 > kMergeN) return RT_ERR_UNSUPPORTED;
    dim3 grid(static_cast<unsigned>((nq + 3) / 4));
    const int64_t total = static_cast<int64_t>(n_lists) * k_in;
    if (total <= 64 * v4::kFinishRegs && k_out <= v4::kFinishCap)
        hipLaunchKernelGGL(topk_merge_select_kernel, grid, dim3(256), 0, st, s, ids, nq, n_lists, k_in, k_out, os, oi);
    else if (total <= 128 && k_out <= 128)
        hipLaunchKernelGGL(topk_merge_regs_kernel<2>, grid, dim3(256), 0, st, s, ids, nq, n_lists, k_in, k_out, os, oi);
    else if (total <= 256 && k_out <= 256)
        hipLaunchKernelGGL(topk_merge_regs_kernel<4>, grid, dim3(256), 0, st, s, ids, nq, n_lists, k_in, k_out, os, oi);
    else
        hipLaunchKernelGGL(topk_merge_kernel, grid, dim3(256), 0, st, s, ids, nq, n_lists, k_in, k_out, os, oi);
    return check_launch("topk_merge_kernel");
}

inline Shape shape_for(int dtype, int d, int k) {
    return dtype == RT_F32 ? shape_f32(d, k) : dtype == RT_F16 ? shape_f16(d, k) : shape_bf16(d, k);
}

constexpr int64_t kCUs = 256;  // MI355X compute units

// planner overrides for tests and tuning (rt_flatip_topk_tuning)
static int g_v4_mode = 0;     // 0 auto, 1 never, 2 wherever legal
static int g_v4_stride = 0;   // 0: planner's choice
static int g_v4_rank = -1;    // -1: planner's choice; 0: no sample (v2-style running threshold)
static int g_v4_joint = 1;    // 1: over several splits, one corpus-wide threshold per query
static int g_dense = 1;       // 1: fp32 small corpora take the GEMM + select pair (topk_dense.h)
static int g_v4_presample = 1;  // 1: joint thresholds from one sample-only launch over every split

// the sample planner (topk_sample_plan.h) restates these; the kernels own them
static_assert(splan::kStageRows == v4::Cfg4<__half, 4>::NT && splan::kStageRows == v4::Cfg4<__half, 8>::NT,
              "sample plan: rows per v4 stage");
static_assert(splan::kMaxK == kMaxK && v4::kMaxK <= kMaxK, "sample plan: the rank table covers every k");
static_assert(splan::kSampleList == v4::kSampleList && v4::kSampleList == 2 * v4::kList,
              "sample plan: group maxima per query");

// v4 (sampled-threshold scan + finish) for 16-bit, d <= 128, 32 < k <= 128 over
// a large corpus with enough queries to fill the chip at <= 8 item splits
inline bool plan_v4(int64_t nq, int64_t nx, int d, int dtype, int k, Plan& p) {
    if (g_v4_mode == 1) return false;
    if (dtype == RT_F32 || d > 128 || k > v4::kMaxK) return false;
    const bool forced = g_v4_mode == 2;
    if (!forced && (k <= v3::kMaxKv3 || nx < 65536)) return false;
    constexpr int QT = v4::Geo<v4::kQS>::QT;
    p.chunk = nq < kQueryChunk ? nq : kQueryChunk;
    if (p.chunk < 1) p.chunk = 1;
    p.q_tiles = static_cast<int>((p.chunk + QT - 1) / QT);
    // enough query tiles that <= kMaxSplits item splits fill the chip (the
    // 8,192-query slice of one of 8 GPUs: 16 tiles x 16 splits)
    if (!forced && static_cast<int64_t>(p.q_tiles) * v4::kMaxSplits < kCUs) return false;
    int splits = 1;
    while (splits < v4::kMaxSplits && static_cast<int64_t>(p.q_tiles) * splits < kCUs) splits *= 2;
    constexpr int NT = v4::Cfg4<__half, 8>::NT;
    int64_t tiles = (nx + NT - 1) / NT;
    while (splits > 1 && tiles / splits < 8) splits /= 2;
    int64_t tiles_per = (tiles + splits - 1) / splits;
    if (tiles_per < 1) tiles_per = 1;
    p.items_per_split = tiles_per * NT;
    p.splits = static_cast<int>(nx > 0 ? (nx + p.items_per_split - 1) / p.items_per_split : 1);
    p.cap = v4::kCap;
    p.v4 = 1;
    // several splits: one threshold per query from a sample of the whole corpus
    // (the union of the splits' buffers then holds ~rank*stride entries, not
    // splits times that); one split: the per-split form
    p.v4_joint = (p.splits > 1 && g_v4_joint) ? 1 : 0;
    p.v4_presample = (p.v4_joint && g_v4_presample) ? 1 : 0;
    // the rows a sample walks as one run of stages: a split (presampled: every
    // split of the corpus; per split: that one alone), or, joint without the
    // presample, the whole corpus
    const int64_t run = (p.v4_joint && !p.v4_presample) ? nx : p.items_per_split;
    const splan::SamplePlan sp = splan::plan_sample_cached(k, p.v4_presample ? nx : run, run);
    p.stride = sp.stride;
    p.rank = sp.rank;
    if (p.v4_presample && (p.stride <= 0 || p.rank <= 0)) p.v4_presample = 0;  // no sample fits: round-4 form
    if (g_v4_stride > 0) p.stride = g_v4_stride;
    if (g_v4_rank >= 0) p.rank = g_v4_rank;
    p.cand_bytes = static_cast<size_t>(p.splits) * v4::q_pad(p) * v4::kCap * sizeof(Cand);
    return true;
}

inline Plan make_plan(int64_t nq, int64_t nx, int d, int dtype, int k, const Shape& sh) {
    Plan p{};
    if (nx > 0 && plan_v4(nq, nx, d, dtype, k, p)) return p;
    if (dtype == RT_F32 && g_dense && dense::applies(nx, d, k)) {
        // the score slab of one query chunk (<= 256 MB: it stays in the Infinity Cache)
        p.dense = 1;
        p.chunk = dense::chunk_for(nq, nx);
        p.q_tiles = 1;
        p.splits = 1;
        p.items_per_split = nx;
        p.cand_bytes = static_cast<size_t>(p.chunk) * dense::ld_for(nx) * sizeof(float);
        return p;
    }
    p.chunk = nq < kQueryChunk ? nq : kQueryChunk;
    if (p.chunk < 1) p.chunk = 1;
    p.q_tiles = static_cast<int>((p.chunk + sh.qt - 1) / sh.qt);
    const int64_t tiles = (nx + sh.nt - 1) / sh.nt;
    int64_t splits;
    if (sh.kind == 2) {
        splits = v2::planned_splits(p.q_tiles, nx);
    } else {
        // at most 2 blocks per CU (<= 512 blocks: one co-resident wave of
        // blocks, no tail), >= 4 item tiles per split, <= 64 splits. C3 (48
        // query tiles x 54 item tiles): 9 splits = 432 blocks run 0.217 ms;
        // rounding up to 11 splits = 528 blocks (3 on some CUs) ran 0.244 ms,
        // 14 splits = 672 blocks 0.243 ms.
        splits = 2 * kCUs / p.q_tiles;
        int64_t max_splits = tiles / 4;
        if (max_splits < 1) max_splits = 1;
        if (splits > max_splits) splits = max_splits;
        if (splits > 64) splits = 64;
        if (splits < 1) splits = 1;
    }
    int64_t tiles_per = (tiles + splits - 1) / splits;
    if (tiles_per < 1) tiles_per = 1;
    p.items_per_split = tiles_per * sh.nt;
    p.splits = static_cast<int>(nx > 0 ? (nx + p.items_per_split - 1) / p.items_per_split : 1);
    p.cap = sh.cap;
    p.kth_bytes = (sh.kind == 0 && p.splits > 1) ? static_cast<size_t>(p.chunk) * sizeof(uint32_t) : 0;
    p.cand_bytes = static_cast<size_t>(p.splits) * p.q_tiles * sh.qt * p.cap * sizeof(Cand);
    p.part_bytes = p.splits > 1 ? static_cast<size_t>(p.splits) * p.chunk * k * (sizeof(float) + sizeof(int64_t)) : 0;
    return p;
}

// The workspace of one call: the byte offset of every region, in this order,
// and their sum. The one place that knows the layout — the size queries, the
// size checks and the pointers of rt_flatip_topk and of the shard entry points
// all come from it. A region starts 256-byte aligned, except that the regions
// after `part` follow its unpadded end (a multiple of 4 bytes; the 4-byte k-th
// keys are all that ever follows a non-empty `part`). The v4 regions hold one
// row per padded query and exist as the plan's flags say.
struct Layout {
    size_t cand;      // candidate buffers (the dense plan: the score slab)
    size_t part;      // per-split partial lists: [split][chunk][k] scores, then ids at part_ids
    size_t part_ids;
    size_t meta;      // v4: per-(split, query, half) entry counts
    size_t kth;       // register lists over several splits: per-query shared k-th keys
    size_t fail;      // v4 joint: per-query rescue flags
    size_t lists;     // v4 presample: [split][q_pad][32] sampled group maxima
    size_t thr;       // v4 presample: per-query thresholds
    size_t total;
};
inline Layout layout_of(const Plan& p) {
    const auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t q_pad = p.v4 ? v4::q_pad(p) : 0;
    Layout l{};
    l.part = l.cand + al(p.cand_bytes);
    l.part_ids = l.part + p.part_bytes / (sizeof(float) + sizeof(int64_t)) * sizeof(float);
    l.meta = l.part + p.part_bytes;
    l.kth = l.meta + al(p.splits * q_pad * 2 * sizeof(int));
    l.fail = l.kth + al(p.kth_bytes);
    l.lists = l.fail + al(p.v4_joint ? q_pad * sizeof(int) : 0);
    l.thr = l.lists + al(p.v4_presample ? p.splits * q_pad * v4::kSampleList * sizeof(float) : 0);
    l.total = l.thr + al(p.v4_presample ? q_pad * sizeof(float) : 0);
    return l;
}
constexpr size_t kWorkspaceSlack = 256;  // the size queries add it to Layout::total

template <typename T>
inline T* region(void* workspace, size_t offset) {
    return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}
// the regions every chunk of a call shares (kth and part: see rt_flatip_topk)
inline void bind_workspace(Args& a, void* workspace, const Layout& l) {
    a.cand = region<Cand>(workspace, l.cand);
    a.meta = region<int>(workspace, l.meta);
    a.fail = region<int>(workspace, l.fail);
    a.v4_lists = region<float>(workspace, l.lists);
    a.v4_thr = region<float>(workspace, l.thr);
}

}  // namespace topk
}  // namespace rt

using namespace rt;

extern "C" size_t rt_flatip_topk_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k) {
    if (nq <= 0 || k <= 0 || k > topk::kMaxK || d <= 0) return 256;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return 256;
    const topk::Plan p = topk::make_plan(nq, nx, d, dtype, k, topk::shape_for(dtype, d, k));
    return topk::layout_of(p).total + topk::kWorkspaceSlack;
}

extern "C" int rt_flatip_topk(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                              int dtype, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                              int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !out_scores || !out_ids || (nx > 0 && !items)) return RT_ERR_INVALID;
    if (k > topk::kMaxK) return RT_ERR_UNSUPPORTED;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (dtype == RT_F32 ? (d % 4 != 0 || d > 256) : (d % 8 != 0 || d > 256)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0xFFFFFFFFll || (id_offset + nx) >= 0xFFFFFFFFll || id_offset < 0) return RT_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(items)) & 15) return RT_ERR_INVALID;
    if (exclude_bits && exclude_words < (nx + 31) / 32) return RT_ERR_INVALID;
    const topk::Plan p = topk::make_plan(nq, nx, d, dtype, k, topk::shape_for(dtype, d, k));
    const topk::Layout lay = topk::layout_of(p);
    if (!workspace || workspace_bytes < lay.total) return RT_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    const size_t esz = dtype == RT_F32 ? 4 : 2;
    for (int64_t q0 = 0; q0 < nq; q0 += p.chunk) {
        const int64_t nc = (nq - q0) < p.chunk ? (nq - q0) : p.chunk;
        float* os = out_scores + q0 * k;
        int64_t* oi = out_ids + q0 * k;
        int rc;
        if (nx == 0) {  // empty corpus: every slot (-FLT_MAX, -1)
            rc = topk::launch_merge(os, oi, nc, 0, 1, k, os, oi, st);
            if (rc) return rc;
            continue;
        }
        topk::Args a{};
        a.Q = reinterpret_cast<const char*>(queries) + q0 * d * esz;
        a.nq = nc;
        a.X = items;
        a.nx = nx;
        a.d = d;
        a.k = k;
        a.excl = exclude_bits ? exclude_bits + q0 * exclude_words : nullptr;
        a.excl_words = exclude_words;
        a.id_offset = id_offset;
        topk::bind_workspace(a, workspace, lay);
        if (p.kth_bytes) {
            a.kth_shared = topk::region<uint32_t>(workspace, lay.kth);
            const hipError_t e = hipMemsetAsync(a.kth_shared, 0, static_cast<size_t>(nc) * sizeof(uint32_t), st);
            if (e != hipSuccess) {
                set_last_error("hipMemsetAsync(topk kth)", e);
                return RT_ERR_HIP;
            }
        }
        if (p.splits > 1 && !p.v4) {  // per-split lists [split][nc][k], merged below
            a.out_s = topk::region<float>(workspace, lay.part);
            a.out_i = topk::region<int64_t>(workspace, lay.part_ids);
        } else {
            a.out_s = os;
            a.out_i = oi;
        }
        switch (dtype) {
            case RT_F32: rc = topk::launch_f32(a, p, st); break;
            case RT_F16: rc = topk::launch_f16(a, p, st); break;
            default: rc = topk::launch_bf16(a, p, st); break;
        }
        if (rc) return rc;
        if (p.splits > 1 && !p.v4) {
            rc = topk::launch_merge(a.out_s, a.out_i, nc, p.splits, k, k, os, oi, st);
            if (rc) return rc;
        }
    }
    return RT_OK;
}

// ---- corpus-sharded search with one corpus-wide threshold per query ----
// (several GPUs, each holding a row shard: rtrec_amd/dist/sharded.py::
// sharded_topk_global). Only where rt_flatip_topk plans the v4 kernel pair.
namespace rt {
namespace topk {
struct ShardArgs {
    Plan p;
    Args a;
    size_t need;
};
// The shard calls presample every split whatever make_plan chose for one GPU,
// and flag nothing (a shard may hold < k of a query's top k): their workspace
// is candidates, meta and sample lists. The threshold region that comes with
// the presample is reserved and unused — the thresholds come from the caller
// (rt_topk_sample_threshold over every shard's lists) — but stays part of the
// reported size.
inline int shard_setup(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype, int k,
                       void* workspace, size_t workspace_bytes, ShardArgs& s) {
    if (nq <= 0 || nx <= 0 || d <= 0 || k <= 0 || k > v4::kMaxK) return RT_ERR_INVALID;
    if (dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_UNSUPPORTED;
    if (d % 8 != 0 || d > 128) return RT_ERR_UNSUPPORTED;
    if (!queries || !items) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(items)) & 15) return RT_ERR_INVALID;
    if (nx >= 0xFFFFFFFFll) return RT_ERR_UNSUPPORTED;
    s.p = make_plan(nq, nx, d, dtype, k, shape_for(dtype, d, k));
    if (!s.p.v4 || s.p.chunk < nq) return RT_ERR_UNSUPPORTED;  // one query chunk, the v4 plan
    s.p.v4_joint = 0;
    s.p.v4_presample = 1;
    const Layout lay = layout_of(s.p);
    s.need = lay.total;
    if (!workspace || workspace_bytes < s.need) return RT_ERR_WORKSPACE;
    s.a = Args{};
    s.a.Q = queries;
    s.a.nq = nq;
    s.a.X = items;
    s.a.nx = nx;
    s.a.d = d;
    s.a.k = k;
    bind_workspace(s.a, workspace, lay);
    return RT_OK;
}
// one scan of the shard in `mode`, with the caller's sample in place of the plan's
inline int shard_scan(int dtype, const Args& a, Plan p, int stride, int rank, int mode, hipStream_t st) {
    p.stride = stride;
    p.rank = rank;
    return dtype == RT_F16 ? v4_scan_f16(a, p, mode, st) : v4_scan_bf16(a, p, mode, st);
}
// {sampled stages, stages} of a shard under plan p (the mode-3 scan of shard_scan)
inline void shard_stage_counts(const Plan& p, int64_t nx, int stride, int64_t* counts) {
    const splan::StageCounts c = splan::sampled_stages(nx, p.items_per_split, stride);
    counts[0] = c.sampled;
    counts[1] = c.total;
}
}  // namespace topk
}  // namespace rt

extern "C" size_t rt_flatip_topk_shard_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k) {
    topk::ShardArgs s{};
    const int rc = topk::shard_setup(reinterpret_cast<const void*>(16), nq, reinterpret_cast<const void*>(16), nx, d,
                                     dtype, k, reinterpret_cast<void*>(16), ~size_t(0), s);
    return rc ? 0 : s.need + topk::kWorkspaceSlack;
}

extern "C" int rt_flatip_topk_shard_plan(int64_t nq, int64_t nx, int d, int dtype, int k, int stride,
                                         int64_t* stage_counts) {
    if (stride < 1 || !stage_counts) return RT_ERR_INVALID;
    topk::ShardArgs s{};
    const int rc = topk::shard_setup(reinterpret_cast<const void*>(16), nq, reinterpret_cast<const void*>(16), nx, d,
                                     dtype, k, reinterpret_cast<void*>(16), ~size_t(0), s);
    if (rc) return rc;
    topk::shard_stage_counts(s.p, nx, stride, stage_counts);
    return RT_OK;
}

extern "C" int rt_flatip_topk_shard_sample(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                                           int dtype, int k, int stride, float* top32, int64_t* stage_counts,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    topk::ShardArgs s{};
    int rc = topk::shard_setup(queries, nq, items, nx, d, dtype, k, workspace, workspace_bytes, s);
    if (rc) return rc;
    if (stride < 1 || !top32 || !stage_counts) return RT_ERR_INVALID;
    topk::shard_stage_counts(s.p, nx, stride, stage_counts);
    hipStream_t st = as_stream(stream);
    topk::Args b = s.a;
    b.lists_out = s.a.v4_lists;
    rc = topk::shard_scan(dtype, b, s.p, stride, 1, 3, st);
    if (rc) return rc;
    return topk::v4::launch_threshold(s.a.v4_lists, s.p.splits, topk::v4::q_pad(s.p) * topk::v4::kSampleList, nq, 1,
                                      nullptr, top32, st);
}

extern "C" int rt_topk_sample_rank(int k, int64_t sampled_stages, int64_t stages, int* rank) {
    if (k <= 0 || k > topk::v4::kMaxK || sampled_stages <= 0 || stages < sampled_stages || !rank) return RT_ERR_INVALID;
    const double f = static_cast<double>(sampled_stages) / static_cast<double>(stages);
    // 0: no failure-safe rank within the lists (the caller scans from -inf)
    *rank = topk::splan::safe_rank(k, f, topk::v4::kSampleList);
    return RT_OK;
}

extern "C" int rt_topk_sample_threshold(const float* lists, int n_lists, int64_t nq, int rank, float* thr,
                                        void* stream) {
    if (!lists || !thr || n_lists <= 0 || nq < 0 || rank < 1 || rank > topk::v4::kSampleList) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    return topk::v4::launch_threshold(lists, n_lists, nq * topk::v4::kSampleList, nq, rank, thr, nullptr,
                                      as_stream(stream));
}

extern "C" int rt_flatip_topk_shard_search(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                                           int dtype, int k, const float* thr, int64_t id_offset, float* out_scores,
                                           int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    topk::ShardArgs s{};
    int rc = topk::shard_setup(queries, nq, items, nx, d, dtype, k, workspace, workspace_bytes, s);
    if (rc) return rc;
    if (!thr || !out_scores || !out_ids || id_offset < 0 || (id_offset + nx) >= 0xFFFFFFFFll) return RT_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    topk::Args b = s.a;
    b.thr_in = thr;
    b.out_s = out_scores;
    b.out_i = out_ids;
    b.id_offset = id_offset;
    rc = topk::shard_scan(dtype, b, s.p, 0, 0, 4, st);
    if (rc) return rc;
    return topk::v4::launch_finish(b, s.p, 3, st);  // no union check: a shard may hold < k
}

extern "C" int rt_flatip_topk_tuning(int v4_mode, int v4_stride, int v4_rank) {
    if (v4_mode < 0 || (v4_mode & 3) > 2 || v4_mode > 30 || v4_stride < 0 || v4_rank < -1 ||
        v4_rank > 2 * topk::v4::kList)
        return RT_ERR_INVALID;
    topk::g_v4_presample = (v4_mode & 16) ? 0 : 1;
    v4_mode &= 15;
    topk::g_dense = (v4_mode & 8) ? 0 : 1;
    v4_mode &= 7;
    topk::g_v4_joint = (v4_mode & 4) ? 0 : 1;
    v4_mode &= 3;
    topk::g_v4_mode = v4_mode;
    topk::g_v4_stride = v4_stride;
    topk::g_v4_rank = v4_rank;
    return RT_OK;
}

extern "C" int rt_topk_merge(const float* scores, const int64_t* ids, int64_t nq, int n_lists, int k_in,
                             int k_out, float* out_scores, int64_t* out_ids, void* stream) {
    if (nq < 0 || n_lists < 0 || k_in <= 0 || k_out <= 0) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!out_scores || !out_ids || (n_lists > 0 && (!scores || !ids))) return RT_ERR_INVALID;
    if (k_out > topk::kMaxK) return RT_ERR_UNSUPPORTED;
    return topk::launch_merge(scores, ids, nq, n_lists, k_in, k_out, out_scores, out_ids, as_stream(stream));
}
