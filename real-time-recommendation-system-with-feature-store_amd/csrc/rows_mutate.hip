// In-place row overwrite and order-preserving row compaction of a dense corpus
// (HBM-bound kernels).
//
// rt_scatter_rows and rt_rows_compact replace the no-op FaissIndex.update /
// FaissIndex.remove of a Flat index (src/serving/retrieval.py:228-246) and give
// the streaming item_update path (-> RetrievalEngine.update_index) an upsert
// and a withdrawal with faiss.IndexFlat.remove_ids ordering: later rows shift
// down, the corpus stays dense, so no search kernel sees a difference.
//
// Rows move as 16-byte vectors with lanes flattened over (row, 16-B chunk),
// nontemporal loads and stores, as in gather.hip.
//
// Compaction is two launches and the kernel boundary is their only inter-block
// ordering (no cross-workgroup hand-off, no wait loop):
//   offsets  one workgroup: a wave popcounts one 2,048-row segment (64 bitmap
//            words, one per lane, the last word masked) per step, then a
//            block-wide exclusive scan with a per-thread carry over the segment
//            counts gives seg_base[0 .. n_seg] in the workspace and n_kept;
//   move     blockIdx.x owns a segment, blockIdx.y a slice of its kept vectors:
//            one thread per bitmap word expands the word into the local indices
//            of its kept rows at the word's in-segment prefix (an LDS list),
//            then the block copies (kept-row rank, chunk) -> dst.
#include "rt_common.h"

namespace rt {
namespace rows {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSegWords = 64;               // one bitmap word per lane of a wave
constexpr int kSegRows = kSegWords * 32;    // 2,048 rows per segment
constexpr int kOffsetsThreads = 1024;
constexpr int kMoveThreads = 256;
// vectors in flight per thread of the move: 4 x 16 B x 256 threads = 16 KiB per
// block, 8 blocks of 4 waves per CU = 128 KiB per CU (the gather's probe note,
// gather.hip:15-17: what matters is independent row reads in flight chip-wide)
constexpr int kMoveUnroll = 4;
constexpr int kMaxSplit = 64;               // slices of one segment (gridDim.y)
constexpr int64_t kMaxRowBytes = 1 << 24;   // (rank, chunk) of a segment stays in 32 bits

// IDX as in gather_rows_kernel: uint32_t when n * vecs_per_row < 2^32, else int64_t
template <typename IDX>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const u32x4* __restrict__ src, int64_t n,
                                                           uint32_t vecs_per_row,
                                                           const int64_t* __restrict__ positions,
                                                           u32x4* __restrict__ dst, int64_t dst_rows,
                                                           int32_t* __restrict__ oob) {
    const IDX total = static_cast<IDX>(n) * vecs_per_row;
    const IDX stride = static_cast<IDX>(gridDim.x) * blockDim.x;
    for (IDX e = static_cast<IDX>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
        const IDX r = e / vecs_per_row;
        const uint32_t c = static_cast<uint32_t>(e - r * vecs_per_row);
        const int64_t p = positions[r];
        if (p >= 0 && p < dst_rows) {
            const u32x4 v = __builtin_nontemporal_load(src + e);  // read once
            __builtin_nontemporal_store(v, dst + p * vecs_per_row + c);
        } else if (c == 0 && oob) {
            atomicAdd(oob, 1);
        }
    }
}

// the keep word `w` with the bits of rows >= n_rows cleared (0 past the bitmap's last word)
__device__ __forceinline__ uint32_t keep_word(const uint32_t* __restrict__ keep_bits, int64_t w, int64_t n_rows) {
    const int64_t row0 = w * 32;
    if (row0 >= n_rows) return 0u;
    uint32_t bits = keep_bits[w];
    const int64_t rem = n_rows - row0;
    if (rem < 32) bits &= (1u << static_cast<uint32_t>(rem)) - 1u;
    return bits;
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < RT_WAVE; o <<= 1) {
        const T t = __shfl_up(v, o, RT_WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ __launch_bounds__(kOffsetsThreads) void compact_offsets_kernel(const uint32_t* __restrict__ keep_bits,
                                                                          int64_t n_rows, int64_t n_seg,
                                                                          int64_t* seg_base, int64_t* n_kept) {
    constexpr int kWaves = kOffsetsThreads / RT_WAVE;
    __shared__ long long wave_total[kWaves];
    const int tid = threadIdx.x, lane = tid & (RT_WAVE - 1), wave = tid / RT_WAVE;
    // segment counts: one wave-wide 256-B read per segment, the reads of four
    // steps issued before the first count is folded (the pass is load latency)
    constexpr int kAhead = 4;
    for (int64_t s0 = wave; s0 < n_seg; s0 += kWaves * kAhead) {
        int c[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int64_t s = s0 + u * kWaves;
            c[u] = s < n_seg ? __popc(keep_word(keep_bits, s * kSegWords + lane, n_rows)) : 0;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c[u] += __shfl_xor(c[u], o, RT_WAVE);
            const int64_t s = s0 + u * kWaves;
            if (lane == 0 && s < n_seg) seg_base[s] = c[u];
        }
    }
    __syncthreads();  // the block's own global writes, read back below
    // exclusive scan in place: thread t carries the contiguous segments [b, e)
    const int64_t chunk = (n_seg + kOffsetsThreads - 1) / kOffsetsThreads;
    const int64_t b = tid * chunk;
    const int64_t e = b + chunk < n_seg ? b + chunk : n_seg;
    long long sum = 0;
    for (int64_t s = b; s < e; ++s) sum += seg_base[s];
    const long long incl = wave_inclusive_scan(sum, lane);
    if (lane == RT_WAVE - 1) wave_total[wave] = incl;
    __syncthreads();
    long long run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    for (int64_t s = b; s < e; ++s) {
        const long long c = seg_base[s];
        seg_base[s] = run;
        run += c;
    }
    if (tid == kOffsetsThreads - 1) {  // its running sum ends at the grand total
        seg_base[n_seg] = run;
        *n_kept = run;
    }
}

__global__ __launch_bounds__(kMoveThreads) void compact_move_kernel(const u32x4* __restrict__ src, int64_t n_rows,
                                                                    uint32_t vecs_per_row,
                                                                    const uint32_t* __restrict__ keep_bits,
                                                                    const int64_t* __restrict__ seg_base,
                                                                    u32x4* __restrict__ dst) {
    __shared__ uint16_t kept_row[kSegRows];  // rank in the segment -> local row index
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    // one thread per word; read before the slice's extent is known, so the bitmap
    // and the segment offsets are one round of loads, not two
    uint32_t bits = tid < kSegWords ? keep_word(keep_bits, seg * kSegWords + tid, n_rows) : 0u;
    const int64_t base = seg_base[seg];
    const uint32_t kept = static_cast<uint32_t>(seg_base[seg + 1] - base);
    const uint32_t total = kept * vecs_per_row;  // <= 2,048 * 2^20
    const uint32_t stride = gridDim.y * kMoveThreads;
    if (blockIdx.y * kMoveThreads >= total) return;  // block-uniform: nothing in this slice
    if (tid < kSegWords) {
        // the 64 words of a segment are one wave, so the in-segment prefix is a
        // wave scan of the popcounts
        const uint32_t c = __popc(bits);
        uint32_t o = wave_inclusive_scan(c, tid) - c;
        while (bits) {
            kept_row[o++] = static_cast<uint16_t>(tid * 32 + __ffs(bits) - 1);
            bits &= bits - 1;
        }
    }
    __syncthreads();
    const u32x4* seg_src = src + seg * kSegRows * static_cast<int64_t>(vecs_per_row);  // 64-bit vector offsets
    u32x4* seg_dst = dst + base * static_cast<int64_t>(vecs_per_row);
    for (uint32_t e0 = blockIdx.y * kMoveThreads + tid; e0 < total; e0 += stride * kMoveUnroll) {
        u32x4 v[kMoveUnroll];
        bool has[kMoveUnroll];
#pragma unroll
        for (int u = 0; u < kMoveUnroll; ++u) {
            // e0 < total <= 2^31 and u * stride <= 3 * 2^14: no 32-bit wrap
            const uint32_t e = e0 + u * stride;
            has[u] = e < total;
            if (has[u]) {
                const uint32_t k = e / vecs_per_row;
                const uint32_t c = e - k * vecs_per_row;
                v[u] = __builtin_nontemporal_load(seg_src + static_cast<int64_t>(kept_row[k]) * vecs_per_row + c);
            }
        }
#pragma unroll
        for (int u = 0; u < kMoveUnroll; ++u)
            if (has[u]) __builtin_nontemporal_store(v[u], seg_dst + (e0 + u * stride));  // kept rows are contiguous in dst
    }
}

inline bool rows_ok(const void* a, const void* b, int64_t row_bytes) {
    return row_bytes > 0 && (row_bytes & 15) == 0 &&
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

inline size_t compact_workspace_bytes(int64_t n_rows) {
    const int64_t n_seg = (n_rows + kSegRows - 1) / kSegRows;
    return (static_cast<size_t>(n_seg + 1) * sizeof(int64_t) + 255) & ~static_cast<size_t>(255);
}

}  // namespace rows
}  // namespace rt

using namespace rt;

extern "C" int rt_scatter_rows(const void* src, int64_t n, int64_t row_bytes, const int64_t* positions, void* dst,
                               int64_t dst_rows, int32_t* oob_count, void* stream) {
    if (n < 0 || dst_rows < 0 || !rows::rows_ok(src, dst, row_bytes)) return RT_ERR_INVALID;
    if (n == 0) return RT_OK;
    if (!src || !positions || (dst_rows > 0 && !dst)) return RT_ERR_INVALID;
    if (row_bytes > rows::kMaxRowBytes) return RT_ERR_UNSUPPORTED;
    const int64_t vpr = row_bytes / 16;
    int64_t blocks = (n * vpr + 255) / 256;
    if (blocks > 0x7FFFFFFF) blocks = 0x7FFFFFFF;  // grid-stride the rest
    const unsigned grid = static_cast<unsigned>(blocks);
    if (n * vpr + static_cast<int64_t>(grid) * 256 < (1ll << 32)) {
        hipLaunchKernelGGL((rows::scatter_rows_kernel<uint32_t>), dim3(grid), dim3(256), 0, as_stream(stream),
                           reinterpret_cast<const rows::u32x4*>(src), n, static_cast<uint32_t>(vpr), positions,
                           reinterpret_cast<rows::u32x4*>(dst), dst_rows, oob_count);
    } else {
        hipLaunchKernelGGL((rows::scatter_rows_kernel<int64_t>), dim3(grid), dim3(256), 0, as_stream(stream),
                           reinterpret_cast<const rows::u32x4*>(src), n, static_cast<uint32_t>(vpr), positions,
                           reinterpret_cast<rows::u32x4*>(dst), dst_rows, oob_count);
    }
    return check_launch("scatter_rows_kernel");
}

extern "C" size_t rt_rows_compact_workspace_bytes(int64_t n_rows) {
    return rows::compact_workspace_bytes(n_rows < 0 ? 0 : n_rows);
}

extern "C" int rt_rows_compact(const void* src, int64_t n_rows, int64_t row_bytes, const uint32_t* keep_bits,
                               int64_t keep_words, void* dst, int64_t dst_rows, int64_t* n_kept, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (n_rows < 0 || dst_rows < n_rows || keep_words < 0 || !rows::rows_ok(src, dst, row_bytes)) return RT_ERR_INVALID;
    if (keep_words < (n_rows + 31) / 32) return RT_ERR_INVALID;
    if (workspace_bytes < rows::compact_workspace_bytes(n_rows)) return RT_ERR_INVALID;
    if (row_bytes > rows::kMaxRowBytes) return RT_ERR_UNSUPPORTED;
    if (n_rows == 0 && !n_kept) return RT_OK;  // nothing to move and nowhere to report it
    if (!n_kept || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return RT_ERR_INVALID;
    if (n_rows > 0) {
        if (!src || !dst || !keep_bits) return RT_ERR_INVALID;
        // out of place: [src, src + n_rows * row_bytes) and [dst, dst + dst_rows * row_bytes) are disjoint
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + static_cast<uintptr_t>(n_rows) * row_bytes;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + static_cast<uintptr_t>(dst_rows) * row_bytes;
        if (s0 < d1 && d0 < s1) return RT_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const int64_t n_seg = (n_rows + rows::kSegRows - 1) / rows::kSegRows;
    if (n_seg > 0x7FFFFFFF) return RT_ERR_UNSUPPORTED;
    int64_t* seg_base = reinterpret_cast<int64_t*>(workspace);
    hipLaunchKernelGGL(rows::compact_offsets_kernel, dim3(1), dim3(rows::kOffsetsThreads), 0, st, keep_bits, n_rows,
                       n_seg, seg_base, n_kept);
    int rc = check_launch("compact_offsets_kernel");
    if (rc != RT_OK || n_seg == 0) return rc;
    const int64_t vpr = row_bytes / 16;
    // slices of a segment: about two unrolled iterations per thread of a full segment
    int64_t split = (rows::kSegRows * vpr + rows::kMoveThreads * rows::kMoveUnroll * 2 - 1) /
                    (rows::kMoveThreads * rows::kMoveUnroll * 2);
    if (split > rows::kMaxSplit) split = rows::kMaxSplit;
    hipLaunchKernelGGL(rows::compact_move_kernel, dim3(static_cast<unsigned>(n_seg), static_cast<unsigned>(split)),
                       dim3(rows::kMoveThreads), 0, st, reinterpret_cast<const rows::u32x4*>(src), n_rows,
                       static_cast<uint32_t>(vpr), keep_bits, seg_base, reinterpret_cast<rows::u32x4*>(dst));
    return check_launch("compact_move_kernel");
}
