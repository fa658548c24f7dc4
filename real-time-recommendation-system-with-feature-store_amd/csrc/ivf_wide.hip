// IVF-Flat wide top-K: rt_ivf_topk's contract for 1 <= k <= 1024
// (rt_ivf_topk_wide). The reference's request path retrieves k =
// num_recommendations * 10 <= 1,000 candidates from its "IVF...,Flat" index
// (src/serving/service.py:206, src/api/schemas.py:21-24); rt_ivf_topk stops at
// 128, the width of the online scan's register sort. The selection here is a
// different one, not that one stretched: a block's partial list is an UNSORTED
// set with a count, and the only sort of a call is the finish's, over the k
// survivors.
//
// Two launches, stream-ordered, no host read, the grid from host arguments only:
//
// 1. ivf_wide_scan: the grid and the window of ivf_scan (rt_ivf_topk_plan,
//    chunk_window), one query per block, the online row stream and
//    online::score_tile unchanged — scores are rt_ivf_topk's bit for bit. After
//    the score:
//      * a block whose window holds <= k rows selects nothing: every row that
//        passes the position and exclusion tests is one composite key (score
//        key << 32 | ~position) stored straight to the block's slice. At the
//        default plan's one-tile chunks that is every block for k >= 256;
//      * a block with a longer window appends keys to an LDS buffer of kCap =
//        2,048 and, whenever a tile ended above kRoom = kCap - 256, compacts it
//        BLOCK-WIDE: every thread holds 8 keys in registers, an 8-bit radix
//        pass is 4 per-wave LDS histograms summed by 256 threads and a suffix
//        scan every wave repeats for itself, passes run from the top byte
//        until the bucket of the k-th best and everything above number <=
//        kKeep = 1,280. The threshold of the next tiles is the lowest score
//        KEPT (ties stay eligible: rows do not arrive in position order). The
//        block's last compaction runs to exactly k.
//    Slice of block (q, lb): slot + 1 words, slot = min(k, rows_per_chunk):
//    [0] the count, [1 .. count] the keys, in no order.
// 2. ivf_wide_finish: one block of 1,024 threads per query over the nprobe x
//    chunks slices. Exact radix select of the k-th largest key, most
//    significant byte first (16 per-wave LDS histograms); the passes read the
//    slices in global memory until the bucket holding the k-th fits the
//    4,096-key LDS bucket, then that bucket. The position bits are part of the
//    key, so a tie group of any size splits by position exactly; copies of
//    one identical key (a row_pos that repeats positions) are cut to k. The
//    <= 1,024 survivors take a bitonic sort in LDS. A second launch, not a
//    last-block ticket: the kernel boundary gives cross-XCD visibility of the
//    slices (topk_online.h).
#include "ivf_select.h"

namespace rt {
namespace topk {
namespace ivfw {

namespace on = rt::topk::online;
namespace iv = rt::topk::ivf;

constexpr int kMaxK = 1024;  // RT_IVF_WIDE_MAX_K
constexpr int kThreads = on::kThreads, kTileRows = on::kTileRows;
constexpr int kCap = 2048;               // keys of a scan block's buffer
constexpr int kRoom = kCap - kTileRows;  // a buffer that passes the check takes one more tile
constexpr int kKeep = 1280;              // a compaction leaves at most this many
constexpr int kPerThread = kCap / kThreads;
static_assert(kCap >= kMaxK + kTileRows, "ivf wide: the buffer holds k keys and one tile of appends");
static_assert(kKeep >= kMaxK && kKeep <= kRoom, "ivf wide: a compaction keeps the k best and leaves room for a tile");
static_assert(kCap % kThreads == 0, "ivf wide: a compaction holds the buffer in registers");

struct ScanLds {
    static constexpr int kStage = on::kWavesS * on::kStageBytes;
    static constexpr int kCand = kCap * 8;
    static constexpr int kQuery = 256 * 4;
    static constexpr int kHist = on::kWavesS * 256 * 4;
    static constexpr int kBytes = kStage + kCand + kQuery + kHist;
};
// 64 B: cnt, thr, ctr[3]; 256 B: the scratch of __syncthreads_or; alignment
static_assert(2 * (ScanLds::kBytes + 64 + 256 + 128) <= 163840, "ivf wide: two blocks per CU");

constexpr int kFinThreads = 1024, kFinWaves = kFinThreads / 64;
constexpr int kBucket = 4096;  // keys of the finish's LDS bucket
static_assert(kMaxK <= kFinThreads && kMaxK <= kBucket, "ivf wide: the finish sorts k keys, one pair per thread");
static_assert(iv::kMaxLists <= kFinThreads, "ivf wide: the finish reads a slice count per thread");
static_assert(kMaxK * 8 + kBucket * 8 + kFinWaves * 256 * 4 + iv::kMaxLists * 4 + 64 <= 65536, "ivf wide: the finish's LDS");

struct Pick {
    int bin, above, inbin;  // the bin of the need-th largest; entries in higher bins; entries in it
};

// wave: hist = 256 summed counts; every lane gets the same Pick. need <= the sum.
__device__ __forceinline__ Pick pick_bin(const uint32_t* hist, int need) {
    const int lane = threadIdx.x & 63;
    const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
    const int c4 = static_cast<int>(h.x + h.y + h.z + h.w);
    int suf = c4;  // inclusive suffix over lanes >= lane (bins ascend with lane)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += t;
    }
    const int ab = suf - c4;
    const int c3 = ab + static_cast<int>(h.w), c2 = c3 + static_cast<int>(h.z);
    const int c1 = c2 + static_cast<int>(h.y), c0 = c1 + static_cast<int>(h.x);
    const bool hit = ab < need && c0 >= need;
    const uint64_t bm = __ballot(hit);
    const int src = bm ? __builtin_ctzll(bm) : 0;
    const int bl = c3 >= need ? 3 : c2 >= need ? 2 : c1 >= need ? 1 : 0;
    const int al = c3 >= need ? ab : c2 >= need ? c3 : c1 >= need ? c2 : c1;
    const int inb = c3 >= need   ? static_cast<int>(h.w)
                    : c2 >= need ? static_cast<int>(h.z)
                    : c1 >= need ? static_cast<int>(h.y)
                                 : static_cast<int>(h.x);
    Pick p;
    p.bin = __shfl(4 * lane + bl, src, 64);
    p.above = __shfl(al, src, 64);
    p.inbin = __shfl(inb, src, 64);
    return p;
}

// block of WAVES waves: one 8-bit pass over the keys each(fn) visits (every key
// once, on some thread) whose bits above `shift` equal `prefix`; the digit is
// bits [shift - 8, shift). hist = WAVES x 256 words. Every thread gets the Pick.
template <int WAVES, class Each>
__device__ __forceinline__ Pick radix_pass(Each&& each, uint32_t* hist, uint64_t prefix, int shift, int need) {
    const int tid = threadIdx.x;
    for (int i = tid; i < WAVES * 256; i += WAVES * 64) hist[i] = 0u;
    __syncthreads();
    const int sh = shift - 8;
    const uint64_t pmask = v4::prefix_mask(shift);
    uint32_t* const mine = hist + (tid >> 6) * 256;
    each([&](uint64_t key) {
        if ((key & pmask) == prefix) atomicAdd(&mine[(key >> sh) & 255u], 1u);
    });
    __syncthreads();
    if (tid < 256) {  // bin tid of every wave's histogram: no other thread touches it
        uint32_t s = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += hist[w * 256 + tid];
        hist[tid] = s;
    }
    __syncthreads();
    const Pick p = pick_bin(hist, need);
    __syncthreads();  // the next pass clears hist
    return p;
}

// block (kThreads): buf[0, n), n > k, keeps in place (in no order) the radix
// bucket of its k-th best and everything above: <= limit keys, the k best among
// them. Copies of one identical key that no pass can tell apart are cut so that
// k keys stay. ctr = 3 LDS words. Returns the new n; lo = the lowest score key
// kept. Every thread of the block calls; ends behind a barrier.
__device__ __forceinline__ int compact_block(uint64_t* buf, int n, int k, int limit, uint32_t* hist, uint32_t* ctr,
                                             uint32_t& lo_out) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint64_t key[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = j * kThreads + tid;
        key[j] = i < n ? buf[i] : 0ull;  // 0 is no key: a position is >= 0, its complement has bit 31 set
    }
    auto each = [&](auto&& fn) {
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
            if (key[j]) fn(key[j]);
    };
    uint64_t prefix = 0ull;
    int shift = 64, need = k, kept = n;
    while (shift > 0) {
        const Pick p = radix_pass<on::kWavesS>(each, hist, prefix, shift, need);
        shift -= 8;
        prefix |= static_cast<uint64_t>(p.bin) << shift;
        need -= p.above;
        kept = (k - need) + p.inbin;
        if (kept <= limit) break;
    }
    if (tid == 0) {
        ctr[0] = 0u;           // keys written back
        ctr[1] = 0u;           // keys equal to the prefix seen (cut only)
        ctr[2] = 0xFFFFFFFFu;  // lowest score key kept
    }
    __syncthreads();  // every key is in registers: the buffer is rewritten from its start
    const uint64_t pmask = v4::prefix_mask(shift);
    const bool cut = kept > limit;  // block-uniform; only with shift == 0: the bucket is copies of one key
    uint32_t lo = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const uint64_t kk = key[j];
        const uint64_t top = kk & pmask;
        bool take = kk != 0ull && top > prefix;
        bool eq = kk != 0ull && top == prefix;
        if (cut) {
            const uint64_t em = __ballot(eq);
            if (em) {
                uint32_t base = 0u;
                if (lane == __builtin_ctzll(em)) base = atomicAdd(&ctr[1], static_cast<uint32_t>(__popcll(em)));
                base = __shfl(base, __builtin_ctzll(em), 64);
                eq = eq && static_cast<int>(base) + ballot_rank(em) < need;
            }
        }
        take = take || eq;
        const uint64_t bm = __ballot(take);
        if (bm) {
            uint32_t base = 0u;
            if (lane == __builtin_ctzll(bm)) base = atomicAdd(&ctr[0], static_cast<uint32_t>(__popcll(bm)));
            base = __shfl(base, __builtin_ctzll(bm), 64);
            const int at = static_cast<int>(base) + ballot_rank(bm);
            if (take && at < kCap) buf[at] = kk;
        }
        if (take) lo = min(lo, static_cast<uint32_t>(kk >> 32));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, static_cast<uint32_t>(__shfl_xor(lo, o, 64)));
    if (lane == 0) atomicMin(&ctr[2], lo);
    __syncthreads();
    lo_out = ctr[2];
    const int m = static_cast<int>(ctr[0]);
    return m < kCap ? m : kCap;
}

// Append the keys of the lanes with `pass` to dst (LDS buffer or the block's
// slice): one LDS atomic per wave, positions by ballot rank. Guarded by cap: a
// row_pos that repeats positions can pass more rows than a window has
// positions. Returns the count this append left (0: nothing appended).
__device__ __forceinline__ int append_key(bool pass, int* cnt, uint64_t* dst, int cap, uint64_t key) {
    const uint64_t bm = __ballot(pass);
    if (!bm) return 0;
    int base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(cnt, __popcll(bm));
    base = __shfl(base, 0, 64);
    const int at = base + ballot_rank(bm);
    if (pass && at < cap) dst[at] = key;
    return base + __popcll(bm);
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void ivf_wide_scan(
    const T* __restrict__ Q, const char* __restrict__ X, int64_t nx, int d, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int64_t* __restrict__ list_len, int64_t n_pos,
    const int32_t* __restrict__ row_pos, const int64_t* __restrict__ probes, int nprobe, int chunks,
    int64_t rows_per_chunk, const uint32_t* __restrict__ excl, int64_t excl_words, int slot,
    uint64_t* __restrict__ slices) {
    constexpr int EPU = 16 / static_cast<int>(sizeof(T));
    constexpr int kStepUnits = on::kStepUnits;
    using L = ScanLds;
    __shared__ __attribute__((aligned(16))) char lds[L::kBytes];
    __shared__ int cnt;
    __shared__ float thr;
    __shared__ uint32_t ctr[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lists = nprobe * chunks;
    const int lb = blockIdx.x, q = blockIdx.y;
    const int p = lb / chunks, c = lb - p * chunks;
    uint64_t* const slice = slices + (static_cast<int64_t>(q) * lists + lb) * (slot + 1);

    on::RowWindow w;
    w.X = X;
    iv::chunk_window(probes[static_cast<int64_t>(q) * nprobe + p], c, list_offsets, nlist, list_len, nx,
                     rows_per_chunk, w.row_begin, w.row_end);
    if (w.row_end <= w.row_begin) {  // block-uniform
        if (threadIdx.x == 0) slice[0] = 0ull;
        return;
    }
    // block-uniform: a window of at most k rows (<= slot: a window is at most a chunk) is written as it is
    const bool direct = (w.row_end - w.row_begin) <= static_cast<int64_t>(k);

    char* const stage = lds + wave * on::kStageBytes;
    uint64_t* const cand = reinterpret_cast<uint64_t*>(lds + L::kStage);
    float* const qs = reinterpret_cast<float*>(lds + L::kStage + L::kCand);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + L::kStage + L::kCand + L::kQuery);
    uint64_t* const dst = direct ? slice + 1 : cand;
    const int cap = direct ? slot : kCap;
    w.units = d / EPU;
    w.row_bytes = static_cast<int64_t>(w.units) * 16;
    w.steps = (w.units + kStepUnits - 1) / kStepUnits;
    w.tiles = static_cast<int>((w.row_end - w.row_begin + kTileRows - 1) / kTileRows);

    for (int e = threadIdx.x; e < d; e += kThreads) qs[e] = to_f32(Q[static_cast<int64_t>(q) * d + e]);
    if (threadIdx.x == 0) {
        cnt = 0;
        thr = -INFINITY;
    }
    uint4 R[kStepUnits];
    on::load_step(R, w, 0, 0);
    __syncthreads();

    int over = 0;  // decided through the barrier that ends a tile: block-uniform (flatip_online_scan)
    for (int t = 0; t < w.tiles; ++t) {
        if (over) {  // never in a direct block
            const int n = cnt < kCap ? cnt : kCap;
            uint32_t lo;
            const int m = compact_block(cand, n, k, kKeep, hist, ctr, lo);
            if (threadIdx.x == 0) {
                cnt = m;
                thr = v2::okey_inv(lo);  // the lowest score kept: an equal later score may win on its position
            }
            __syncthreads();
        }
        const float th = thr;
        const int64_t row = w.row_begin + static_cast<int64_t>(t) * kTileRows + wave * 64 + lane;
        const int32_t pos = row < w.row_end ? row_pos[row] : -1;  // in flight under the scores

        float acc[1];
        on::score_tile<T, 1>(R, w, t, stage, qs, d, acc);

        bool pass = iv::pos_passes(pos, n_pos, acc[0], th);
        if (excl && pass) pass = iv::bitmap_clear(excl, excl_words, q, pos);
        const uint64_t key = v4::ckey(Cand{acc[0], static_cast<uint32_t>(pos)});
        const int after = append_key(pass, &cnt, dst, cap, key);
        over = __syncthreads_or((!direct && after > kRoom) ? 1 : 0);
    }

    if (direct) {
        if (threadIdx.x == 0) slice[0] = static_cast<uint64_t>(cnt < slot ? cnt : slot);
        return;
    }
    int n = cnt < kCap ? cnt : kCap;
    if (n > k) {  // block-uniform
        uint32_t lo;
        n = compact_block(cand, n, k, k, hist, ctr, lo);
    }
    if (n > slot) n = slot;  // cannot happen: a window longer than k has slot == k
    for (int i = threadIdx.x; i < n; i += kThreads) slice[1 + i] = cand[i];
    if (threadIdx.x == 0) slice[0] = static_cast<uint64_t>(n);
}

__global__ __launch_bounds__(kFinThreads) void ivf_wide_finish(const uint64_t* __restrict__ slices, int lists, int slot,
                                                               int k, float* __restrict__ out_s,
                                                               int64_t* __restrict__ out_i) {
    __shared__ __attribute__((aligned(16))) uint64_t keep[kMaxK];
    __shared__ __attribute__((aligned(16))) uint64_t bucket[kBucket];
    __shared__ __attribute__((aligned(16))) uint32_t hist[kFinWaves * 256];
    __shared__ int cnts[iv::kMaxLists];
    __shared__ int ctr[4];  // keys in all slices; keys in keep; keys in bucket; keys equal to the k-th taken
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const uint64_t* const base = slices + static_cast<int64_t>(q) * lists * (slot + 1);
    if (tid < 4) ctr[tid] = 0;
    keep[tid] = 0ull;
    __syncthreads();
    if (tid < lists) {
        const uint64_t c = base[static_cast<int64_t>(tid) * (slot + 1)];
        const int ci = c < static_cast<uint64_t>(slot) ? static_cast<int>(c) : slot;
        cnts[tid] = ci;
        if (ci) atomicAdd(&ctr[0], ci);
    }
    __syncthreads();
    const int total = ctr[0];

    // a wave per slice, a lane per key: coalesced
    auto each_global = [&](auto&& fn) {
        for (int s = wave; s < lists; s += kFinWaves) {
            const int c = cnts[s];
            const uint64_t* const ks = base + static_cast<int64_t>(s) * (slot + 1) + 1;
            for (int i = lane; i < c; i += 64) fn(ks[i]);
        }
    };
    auto to_keep = [&](uint64_t key) {
        const int at = atomicAdd(&ctr[1], 1);
        if (at < kMaxK) keep[at] = key;
    };

    if (total <= k) {
        each_global(to_keep);
    } else {
        int nb = 0;
        auto each_bucket = [&](auto&& fn) {
            for (int i = tid; i < nb; i += kFinThreads) fn(bucket[i]);
        };
        uint64_t prefix = 0ull;
        int shift = 64, need = k, bcount = total;
        bool staged = false;  // every value that steers this loop is block-uniform
        for (;;) {
            if (!staged && bcount <= kBucket) {
                // the bucket of the k-th fits: what is above it is in the result, the bucket moves to LDS
                const uint64_t pmask = v4::prefix_mask(shift);
                each_global([&](uint64_t key) {
                    const uint64_t top = key & pmask;
                    if (top > prefix) to_keep(key);
                    else if (top == prefix) {
                        const int at = atomicAdd(&ctr[2], 1);
                        if (at < kBucket) bucket[at] = key;
                    }
                });
                __syncthreads();
                nb = ctr[2] < kBucket ? ctr[2] : kBucket;
                staged = true;
            }
            if (shift == 0 || bcount == need) break;  // the k-th key itself, or a bucket taken whole
            const Pick p = staged ? radix_pass<kFinWaves>(each_bucket, hist, prefix, shift, need)
                                  : radix_pass<kFinWaves>(each_global, hist, prefix, shift, need);
            shift -= 8;
            prefix |= static_cast<uint64_t>(p.bin) << shift;
            need -= p.above;
            bcount = p.inbin;
        }
        // above the k-th: taken; equal to it (copies of one key when shift == 0): `need` of them
        const uint64_t pmask = v4::prefix_mask(shift);
        auto take = [&](uint64_t key) {
            const uint64_t top = key & pmask;
            bool t = top > prefix;
            if (top == prefix) t = atomicAdd(&ctr[3], 1) < need;
            if (t) to_keep(key);
        };
        if (staged) each_bucket(take);
        else each_global(take);  // more than kBucket copies of one key
    }
    __syncthreads();

    // bitonic sort, descending, of the first n2 >= k slots (0 = none sorts last)
    int n2 = 2;
    while (n2 < k) n2 <<= 1;
    for (int sz = 2; sz <= n2; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            if (tid < (n2 >> 1)) {
                const int i = 2 * tid - (tid & (st - 1)), j = i + st;
                const bool desc = (i & sz) == 0;
                const uint64_t a = keep[i], b = keep[j];
                if ((a < b) == desc && a != b) {
                    keep[i] = b;
                    keep[j] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid < k) {
        const uint64_t key = keep[tid];
        const int64_t o = static_cast<int64_t>(q) * k + tid;
        out_s[o] = key ? v2::okey_inv(static_cast<uint32_t>(key >> 32)) : -FLT_MAX;
        out_i[o] = key ? static_cast<int64_t>(~static_cast<uint32_t>(key)) : -1ll;
    }
}

}  // namespace ivfw
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace iw = rt::topk::ivfw;

static_assert(RT_IVF_WIDE_MAX_K == iw::kMaxK, "rtrec_hip.h restates the kernel's limit");

// slot: the keys a block's slice holds
static int64_t wide_slot(int k, int64_t rows_per_chunk) { return k < rows_per_chunk ? k : rows_per_chunk; }

extern "C" size_t rt_ivf_topk_wide_workspace_bytes(int64_t nq, int nprobe, int64_t max_list_rows, int k) {
    int64_t plan[3];
    if (k <= 0 || k > iw::kMaxK || rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK) return 256;
    const size_t need = static_cast<size_t>(plan[2]) * static_cast<size_t>(wide_slot(k, plan[1]) + 1) * sizeof(uint64_t);
    return need < 256 ? 256 : need;
}

extern "C" int rt_ivf_topk_wide(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                                const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                                const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows,
                                int k, const uint32_t* exclude_bits, int64_t exclude_words, float* out_scores,
                                int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0 || n_pos < 0)
        return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !out_scores || !out_ids || !list_offsets || !probes || (nx > 0 && (!rows || !row_pos)))
        return RT_ERR_INVALID;
    if (k > iw::kMaxK || nprobe > iw::iv::kMaxProbe || nq > iw::iv::kMaxNq) return RT_ERR_UNSUPPORTED;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!iw::on::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll || n_pos >= 0x7FFFFFFFll || max_list_rows >= 0xFFFFFFFFll)
        return RT_ERR_UNSUPPORTED;  // positions are int32
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(rows)) & 15) return RT_ERR_INVALID;
    if (exclude_bits && exclude_words < (n_pos + 31) / 32) return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < rt_ivf_topk_wide_workspace_bytes(nq, nprobe, max_list_rows, k))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return RT_ERR_INVALID;
    int64_t plan[3];
    if (rt_ivf_topk_plan(nq, nprobe, max_list_rows, plan) != RT_OK) return RT_ERR_UNSUPPORTED;
    const int chunks = static_cast<int>(plan[0]);
    const int64_t rows_per_chunk = plan[1];
    const int lists = nprobe * chunks;
    const int slot = static_cast<int>(wide_slot(k, rows_per_chunk));
    hipStream_t st = as_stream(stream);
    uint64_t* slices = static_cast<uint64_t*>(workspace);
    const dim3 grid(static_cast<unsigned>(lists), static_cast<unsigned>(nq)), block(iw::kThreads);
    const char* x = static_cast<const char*>(rows);
#define RT_IVF_WIDE_LAUNCH(T)                                                                                      \
    hipLaunchKernelGGL((iw::ivf_wide_scan<T>), grid, block, 0, st, static_cast<const T*>(queries), x, nx, d, k,     \
                       list_offsets, nlist, list_len, n_pos, row_pos, probes, nprobe, chunks, rows_per_chunk,       \
                       exclude_bits, exclude_words, slot, slices)
    switch (dtype) {
        case RT_F32: RT_IVF_WIDE_LAUNCH(float); break;
        case RT_F16: RT_IVF_WIDE_LAUNCH(__half); break;
        default: RT_IVF_WIDE_LAUNCH(__hip_bfloat16); break;
    }
#undef RT_IVF_WIDE_LAUNCH
    int rc = check_launch("ivf_wide_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(iw::ivf_wide_finish, dim3(static_cast<unsigned>(nq)), dim3(iw::kFinThreads), 0, st, slices,
                       lists, slot, k, out_scores, out_ids);
    return check_launch("ivf_wide_finish");
}
