// Host arithmetic of the list-major IVF batch search (ivf_batch.hip): the row
// chunks of a probed list, the host bound of the work items and the workspace
// formula. No device code and no HIP header: ivf_batch.hip includes it, and
// tests/ivf_batch_plan_main.cpp compiles it with plain g++ under ASan/UBSan
// (tests/test_ivf_batch_abi_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace rt {
namespace topk {
namespace ivfb {

constexpr int kQT = 32;            // queries of a work item: one 32x32 MFMA tile
constexpr int kTileRows = 128;     // rows a block scores between two compaction checks (4 waves x 32)
constexpr int kMaxLists = 512;     // partial lists per query the finish takes (online::kMaxBlocks)
constexpr int kMaxK = 128;         // RT_IVF_MAX_K
constexpr int kMaxProbe = 128;     // RT_IVF_MAX_NPROBE
// A chunk is 8 tiles (1,024 rows, the mean list of the default 1M x IVF1024
// index) unless the finish's 512 lists force a longer one: a work item stages
// its 32 queries and writes 32 partial lists once per chunk — fixed costs that a
// longer chunk spreads — while every chunk of the LONGEST list costs each query
// nprobe partial lists of workspace, whatever the length of its own lists. A
// policy value, not a measured one.
constexpr int kChunkTiles = 8;

struct Plan {
    int qt;                  // queries per work item
    int64_t rows_per_chunk;  // a multiple of kTileRows
    int chunks;              // per probed list; nprobe x chunks <= kMaxLists
    int64_t items_bound;     // host bound of the work items (list, query tile, chunk)
    int64_t blocks;          // scan blocks launched (= items_bound: surplus blocks leave)
};

// false: a refused shape (the caller has checked nq, nprobe, nlist, k > 0 and max_list_rows >= 0)
inline bool make_plan(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows, int k, Plan& p) {
    if (nq <= 0 || nprobe <= 0 || nlist <= 0 || max_list_rows < 0 || k <= 0) return false;
    if (nprobe > kMaxProbe || k > kMaxK || nlist >= 0x7FFFFFFFll || max_list_rows >= 0xFFFFFFFFll) return false;
    if (nq >= 0x7FFFFFFFll / nprobe) return false;  // pairs are int32
    const int64_t pairs = nq * nprobe;
    const int64_t tile = kTileRows;
    const int64_t mlr = max_list_rows > 0 ? max_list_rows : 1;
    const int64_t cap = kMaxLists / nprobe;  // >= 4 chunks per list
    const int64_t tiles = (mlr + tile - 1) / tile;
    int64_t tpc = (tiles + cap - 1) / cap;  // tiles per chunk, at least
    const int64_t want = tiles < kChunkTiles ? tiles : kChunkTiles;
    if (tpc < want) tpc = want;
    p.qt = kQT;
    p.rows_per_chunk = tpc * tile;
    p.chunks = static_cast<int>((mlr + p.rows_per_chunk - 1) / p.rows_per_chunk);
    // sum over lists of ceil(c_l / QT) <= floor(P / QT) + (lists with a pair) <= P / QT + min(nlist, P)
    p.items_bound = (pairs / kQT + (nlist < pairs ? nlist : pairs)) * p.chunks;
    p.blocks = p.items_bound;
    return p.blocks < 0x7FFFFFFFll;  // grid.x
}

// [partial lists: nq x k x nprobe x chunks composite keys of 8 bytes]
// [int32: counts nlist | pair starts nlist + 1 | tile starts nlist + 1 | rank P | pairs P], P = nq x nprobe;
// rounded up to 256. Monotone in nq: chunks does not depend on it.
inline size_t partial_bytes(int64_t nq, int nprobe, int k, const Plan& p) {
    return static_cast<size_t>(nq) * static_cast<size_t>(k) * static_cast<size_t>(nprobe) *
           static_cast<size_t>(p.chunks) * 8u;
}
inline size_t workspace_bytes(int64_t nq, int nprobe, int64_t nlist, int k, const Plan& p) {
    const size_t ints = 3u * static_cast<size_t>(nlist) + 2u + 2u * static_cast<size_t>(nq) * static_cast<size_t>(nprobe);
    const size_t need = partial_bytes(nq, nprobe, k, p) + 4u * ints;
    return (need + 255u) / 256u * 256u;
}

}  // namespace ivfb
}  // namespace topk
}  // namespace rt
