// What the probed-list scans share (ivf_scan, ivf.hip; ivf_pq_scan, ivf_pq.hip):
// the limits and the plan of the (probe x chunk, query) grid, the window of a
// block, the position tests of the selection and the compaction that keeps
// ties. The scans differ in how a row gets its score, in nothing after it.
#pragma once
#include "topk_online.h"

namespace rt {
namespace topk {
namespace ivf {

namespace on = rt::topk::online;

constexpr int kMaxProbe = 128;                // RT_IVF_MAX_NPROBE
constexpr int kMaxLists = on::kMaxBlocks;     // partial lists per query the finish takes (one thread each)
constexpr int64_t kMaxNq = 65535;             // grid.y
static_assert(kMaxProbe <= kMaxLists, "ivf: one partial list per probe at least");

struct Plan {
    int chunks;              // per probed list
    int64_t rows_per_chunk;  // a multiple of the scan's 256-row tile
};

// Smallest chunks (>= min_tiles tiles) that keep nprobe x chunks within the
// finish's 512 lists: at nq = 1 the blocks of a call are all the parallelism
// there is (20 probes of ~1,000 rows = 80 blocks of one tile, not 20).
inline Plan make_plan(int nprobe, int64_t max_list_rows, int min_tiles) {
    const int64_t tile = on::kTileRows;
    const int64_t mlr = max_list_rows > 0 ? max_list_rows : 1;
    const int64_t cap = kMaxLists / (nprobe > 0 ? nprobe : 1);  // >= 4
    int64_t tiles = (mlr + tile - 1) / tile;
    int64_t tpc = (tiles + cap - 1) / cap;  // tiles per chunk
    if (tpc < min_tiles) tpc = min_tiles;
    Plan p;
    p.rows_per_chunk = tpc * tile;
    p.chunks = static_cast<int>((mlr + p.rows_per_chunk - 1) / p.rows_per_chunk);
    return p;
}

// wave: compact one candidate buffer; thr = the lowest score kept
__device__ __forceinline__ void compact_keep_ties(Cand* buf, int& n, int k, int limit, uint32_t* hist, float& thr) {
    const int lane = threadIdx.x & 63;
    float unused = 0.f;
    v4::compact_stream(buf, n, k, limit, hist, unused);
    wave_lds_sync();
    float lo = INFINITY;
    for (int i = lane; i < n; i += 64) lo = fminf(lo, buf[i].s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    thr = lo;
}

// Chunk c of probe entry l, clamped to the list and to the corpus: the stored
// rows [begin, end), begin == end == 0 when nothing is left (l == -1 or outside
// [0, nlist), an empty list, a chunk past the list's end). list_len != nullptr:
// lists with slack, the first list_len[l] rows of the capacity.
__device__ __forceinline__ void chunk_window(int64_t l, int c, const int64_t* __restrict__ list_offsets, int64_t nlist,
                                             const int64_t* __restrict__ list_len, int64_t nx, int64_t rows_per_chunk,
                                             int64_t& begin, int64_t& end) {
    begin = end = 0;
    if (l >= 0 && l < nlist) {
        int64_t lo = list_offsets[l], hi = list_offsets[l + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > nx ? nx : hi;
        if (list_len && lo < hi) {
            const int64_t live = list_len[l];
            hi = live <= 0 ? lo : (live < hi - lo ? lo + live : hi);
        }
        if (lo < hi) {
            const int64_t len = hi - lo, first = static_cast<int64_t>(c) * rows_per_chunk;
            if (first < len) {
                begin = lo + first;
                end = (first + rows_per_chunk) < len ? (begin + rows_per_chunk) : hi;
            }
        }
    }
}

// block: the partial list of a block with no row to scan, every rank "none"
__device__ __forceinline__ void write_none(uint64_t* out, int k, int lists) {
    for (int r = threadIdx.x; r < k; r += on::kThreads) out[static_cast<int64_t>(r) * lists] = 0ull;
}

// A position outside [0, n_pos) (a corrupt row_pos, an empty slot of a list with
// slack) is dropped: it has no bit in the bitmap and no row in the caller's corpus.
__device__ __forceinline__ bool pos_passes(int32_t pos, int64_t n_pos, float score, float thr) {
    return pos >= 0 && static_cast<int64_t>(pos) < n_pos && score >= thr;
}

// the dense exclusion bitmap, indexed by ORIGINAL position
__device__ __forceinline__ bool bitmap_clear(const uint32_t* __restrict__ excl, int64_t excl_words, int q,
                                             int32_t pos) {
    return ((excl[static_cast<int64_t>(q) * excl_words + (pos >> 5)] >> (pos & 31)) & 1u) == 0u;
}

}  // namespace ivf
}  // namespace topk
}  // namespace rt
