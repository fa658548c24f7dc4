// What the list-major batch scans share (ivfb_scan, ivf_batch.hip; ivf_sq8b_scan,
// ivf_sq8_batch.hip): the four grouping launches and their launch code, the
// workspace tables, the work item of a scan block and everything behind the
// score — the per-query threshold, the LDS candidate buffers with compaction,
// the sorted partial lists. The scans differ in how a (query, row) pair gets its
// score, in nothing before or after it.
#pragma once
#include "ivf_batch_plan.h"
#include "ivf_select.h"

namespace rt {
namespace topk {
namespace ivfb {

namespace on = rt::topk::online;

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kCap = 320;           // candidate buffer of one query
constexpr int kRoom = kCap - kTileRows;
static_assert(kTileRows == 32 * kWaves, "ivf batch: a wave scores one 32-row MFMA tile per step");
static_assert(kRoom >= kMaxK, "ivf batch: a compaction must be able to keep the k best");
static_assert(kMaxK <= v4::kFinishCap, "ivf batch: the block's list is sorted by the 128-entry register sort");
static_assert(kMaxLists == on::kMaxBlocks && kMaxK == on::kMaxK, "ivf_batch_plan.h restates the finish's limits");

// which of {grouping, scan, finish} a call issues (rt_ivf_topk_batch_tuning, ivf_batch.hip)
int stages();

// zero `bytes` (a multiple of 4) from an 8-byte aligned base: the partial lists and the counts
static __global__ __launch_bounds__(256) void ivfb_zero(uint64_t* __restrict__ base, size_t bytes) {
    const size_t n8 = bytes / 8;
    const size_t step = static_cast<size_t>(gridDim.x) * 256;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n8; i += step) base[i] = 0ull;
    if ((bytes & 4) && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<uint32_t*>(base)[2 * n8] = 0u;
}

static __global__ __launch_bounds__(256) void ivfb_count(const int64_t* __restrict__ probes, int64_t pairs,
                                                         int64_t nlist, int32_t* __restrict__ count,
                                                         int32_t* __restrict__ rank) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int64_t l = probes[p];
    rank[p] = (l >= 0 && l < nlist) ? atomicAdd(&count[l], 1) : -1;
}

// one block: thread t owns the lists [t seg, (t + 1) seg)
static __global__ __launch_bounds__(1024) void ivfb_offsets(const int32_t* __restrict__ count, int64_t nlist,
                                                            int32_t* __restrict__ pair_start,
                                                            int32_t* __restrict__ tile_start) {
    __shared__ int sp[1024], st[1024];
    const int t = threadIdx.x;
    const int64_t seg = (nlist + 1023) / 1024;
    const int64_t a = t * seg < nlist ? t * seg : nlist, b = (a + seg) < nlist ? (a + seg) : nlist;
    int np = 0, nt = 0;
    for (int64_t l = a; l < b; ++l) {
        const int c = count[l];
        np += c;
        nt += (c + kQT - 1) / kQT;
    }
    sp[t] = np;
    st[t] = nt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int up = t >= o ? sp[t - o] : 0, ut = t >= o ? st[t - o] : 0;
        __syncthreads();
        sp[t] += up;
        st[t] += ut;
        __syncthreads();
    }
    int bp = sp[t] - np, bt = st[t] - nt;
    for (int64_t l = a; l < b; ++l) {
        const int c = count[l];
        pair_start[l] = bp;
        tile_start[l] = bt;
        bp += c;
        bt += (c + kQT - 1) / kQT;
    }
    if (t == 1023) {
        pair_start[nlist] = sp[t];
        tile_start[nlist] = st[t];
    }
}

static __global__ __launch_bounds__(256) void ivfb_scatter(const int64_t* __restrict__ probes, int64_t pairs,
                                                           int64_t nlist, const int32_t* __restrict__ pair_start,
                                                           const int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ out) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int64_t l = probes[p];
    const int r = rank[p];
    // probes may change between two launches of a call only by the caller's error: the
    // slot is tested all the same, so that nothing is written outside `out`
    if (l >= 0 && l < nlist && r >= 0) {
        const int64_t at = static_cast<int64_t>(pair_start[l]) + r;
        if (at < pairs) out[at] = static_cast<int32_t>(p);
    }
}

// the workspace of a call: the partial lists, then the grouping tables (ivf_batch_plan.h)
struct Tables {
    uint64_t* partials;
    size_t pbytes;
    int32_t *count, *pair_start, *tile_start, *rank, *pair_of;
};

inline Tables carve(void* workspace, int64_t nq, int nprobe, int64_t nlist, int k, const Plan& p) {
    Tables t;
    t.pbytes = partial_bytes(nq, nprobe, k, p);
    t.partials = static_cast<uint64_t*>(workspace);
    t.count = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + t.pbytes);
    t.pair_start = t.count + nlist;
    t.tile_start = t.pair_start + nlist + 1;
    t.rank = t.tile_start + nlist + 1;
    t.pair_of = t.rank + nq * nprobe;
    return t;
}

// the fill and the three grouping launches
inline int launch_grouping(const Tables& t, const int64_t* probes, int64_t pairs, int64_t nlist, hipStream_t st) {
    // the partial lists and the counts lie side by side: one fill launch
    const size_t zbytes = t.pbytes + static_cast<size_t>(nlist) * 4;
    const size_t zblocks = (zbytes / 8 + 2047) / 2048;  // 8 words per thread, at most
    hipLaunchKernelGGL(ivfb_zero, dim3(static_cast<unsigned>(zblocks < 1 ? 1 : (zblocks > 4096 ? 4096 : zblocks))),
                       dim3(256), 0, st, t.partials, zbytes);
    int rc = check_launch("ivfb_zero");
    if (rc) return rc;
    const unsigned pblocks = static_cast<unsigned>((pairs + 255) / 256);
    hipLaunchKernelGGL(ivfb_count, dim3(pblocks), dim3(256), 0, st, probes, pairs, nlist, t.count, t.rank);
    rc = check_launch("ivfb_count");
    if (rc) return rc;
    hipLaunchKernelGGL(ivfb_offsets, dim3(1), dim3(1024), 0, st, t.count, nlist, t.pair_start, t.tile_start);
    rc = check_launch("ivfb_offsets");
    if (rc) return rc;
    hipLaunchKernelGGL(ivfb_scatter, dim3(pblocks), dim3(256), 0, st, probes, pairs, nlist, t.pair_start, t.rank,
                       t.pair_of);
    return check_launch("ivfb_scatter");
}

// The work item of scan block b = (tile number T = b / chunks, chunk c = b % chunks).
struct Item {
    int64_t p0;                  // the tile's pairs are pairs[p0, p0 + nqt)
    int nqt;                     // 1..kQT
    int c;                       // chunk of the list
    int64_t row_begin, row_end;  // the chunk, clamped to the list and to the corpus (ivf_scan's window)
};

// false (block-uniform): a surplus block of the host bound, or a chunk with no
// row, leaves — the partial lists were zeroed. The tables are this call's own
// (ivfb_offsets), and consistent ones give 0 <= p0 < p1 <= n_pairs; the block
// tests it all the same (in 64 bits), and every pair id later, so that no table
// contents can take a read outside `pairs` or a write outside the partial lists.
__device__ __forceinline__ bool work_item(const int32_t* __restrict__ pair_start,
                                          const int32_t* __restrict__ tile_start, int n_pairs, int chunks,
                                          const int64_t* __restrict__ list_offsets, int64_t nlist,
                                          const int64_t* __restrict__ list_len, int64_t nx, int64_t rows_per_chunk,
                                          Item& w) {
    const int T_ = static_cast<int>(blockIdx.x / static_cast<unsigned>(chunks));
    w.c = static_cast<int>(blockIdx.x - static_cast<unsigned>(T_) * static_cast<unsigned>(chunks));
    if (T_ >= tile_start[nlist]) return false;
    int64_t lo = 0, hi = nlist - 1;  // the first list with tile_start[l + 1] > T_ (one exists)
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tile_start[mid + 1] > T_) hi = mid;
        else lo = mid + 1;
    }
    const int64_t l = lo;
    w.p0 = pair_start[l] + (static_cast<int64_t>(T_) - tile_start[l]) * kQT;
    int64_t p1 = pair_start[l + 1];
    p1 = p1 < n_pairs ? p1 : n_pairs;
    if (w.p0 < 0 || w.p0 >= p1) return false;
    w.nqt = (p1 - w.p0) < kQT ? static_cast<int>(p1 - w.p0) : kQT;
    ivf::chunk_window(l, w.c, list_offsets, nlist, list_len, nx, rows_per_chunk, w.row_begin, w.row_end);
    return w.row_end > w.row_begin;
}

// threads 0..kQT-1: the tile's slots. qid = -1: no query in this slot of the tile.
__device__ __forceinline__ void tile_slots(const Item& w, const int32_t* __restrict__ pairs, int n_pairs, int nprobe,
                                           int* qid, int* qslot, int* cnt, float* thr) {
    const int tid = threadIdx.x;
    if (tid < kQT) {
        int pid = -1;
        if (tid < w.nqt) pid = pairs[w.p0 + tid];
        const bool ok = pid >= 0 && pid < n_pairs;
        const int q = ok ? pid / nprobe : -1;
        qid[tid] = q;
        qslot[tid] = ok ? pid - q * nprobe : 0;
        cnt[tid] = 0;
        thr[tid] = -INFINITY;
    }
}

// Selection of one scored tile: acc[r] = (query tile_row(r, half), row `col` of
// this wave), `valid` = the lane's row is inside the window and its position
// inside [0, n_pos). A score at or above its query's threshold whose position
// passes the bitmap is appended to the query's buffer, one LDS atomic per lane
// half (the halves hold different queries). Returns whether a buffer this lane
// appended to went above kRoom.
__device__ __forceinline__ int select_tile(const f32x16& acc, bool valid, int32_t pos, const int* qid,
                                           const float* thr, int* cnt, Cand* cand,
                                           const uint32_t* __restrict__ excl, int64_t excl_words) {
    const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    int mine_over = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qi = tile_row(r, half);
        bool pass = valid && qid[qi] >= 0 && acc[r] >= thr[qi];
        if (excl && pass)
            pass = ((excl[static_cast<int64_t>(qid[qi]) * excl_words + (pos >> 5)] >> (pos & 31)) & 1u) == 0u;
        const uint64_t bm = __ballot(pass);
        if (bm) {  // wave-uniform
            const uint32_t mine = half ? static_cast<uint32_t>(bm >> 32) : static_cast<uint32_t>(bm);
            const int n_mine = __popc(mine);
            int base = 0;
            if (col == 0 && n_mine) base = atomicAdd(&cnt[qi], n_mine);
            base = __shfl(base, half * 32, 64);
            const int at = base + __popc(mine & ((1u << col) - 1u));
            // guarded: a row_pos that repeats positions gives equal keys, of which a
            // compaction may keep more than its limit
            if (pass && at < kCap) cand[qi * kCap + at] = Cand{acc[r], static_cast<uint32_t>(pos)};
            mine_over |= (base + n_mine) > kRoom ? 1 : 0;
        }
    }
    return mine_over;
}

// block, after the barrier that found a buffer above kRoom: wave w compacts the
// buffers of slots w, w + 4, ...; the threshold after a compaction is the lowest
// score kept, because rows do not arrive in position order. Down to the finish's
// 128, not to kRoom: a buffer left near kRoom passes the check again after the
// next tile's first appends.
__device__ __forceinline__ void compact_tile_buffers(int nqt, int k, int* cnt, float* thr, Cand* cand,
                                                     uint32_t* hist) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int qi = wave; qi < nqt; qi += kWaves) {
        int n = cnt[qi] < kCap ? cnt[qi] : kCap;
        if (n > kRoom) {
            float th = thr[qi];
            ivf::compact_keep_ties(cand + qi * kCap, n, k, v4::kFinishCap, hist, th);
            if (lane == 0) {
                cnt[qi] = n;
                thr[qi] = th;
            }
        }
    }
}

// block: every query's list goes out sorted, as composite keys, to
// partials[query][rank][slot x chunks + c] — the format of the per-query scan
__device__ __forceinline__ void write_tile_lists(const Item& w, int k, int nprobe, int chunks, const int* qid,
                                                 const int* qslot, const int* cnt, Cand* cand, uint32_t* hist,
                                                 uint64_t* __restrict__ partials) {
    const int wave = threadIdx.x >> 6;
    const int lists = nprobe * chunks;
    for (int qi = wave; qi < w.nqt; qi += kWaves) {
        if (qid[qi] < 0) continue;  // wave-uniform
        const int n = cnt[qi] < kCap ? cnt[qi] : kCap;
        on::write_block_list(cand + qi * kCap, n, k, hist,
                             partials + static_cast<int64_t>(qid[qi]) * k * lists + qslot[qi] * chunks + w.c, lists);
    }
}

}  // namespace ivfb
}  // namespace topk
}  // namespace rt
