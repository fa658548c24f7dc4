// rt_tag_filter_bitmap: the tag filter (topk_online.h: per-item 64-bit category
// sets, per-query any_of / none_of masks) as an exclusion bitmap, for the paths
// that take a bitmap and have no native filter: rt_flatip_topk,
// rt_ivf_topk_batch, and calls above the limits of the resident searchers. Serves
// the request schema's filter_categories (src/api/schemas.py:21-34).
//
// A block of 256 threads produces 256 words (8,192 items) of one query's row. In
// each of 32 rounds a thread loads ONE tag — consecutive lanes, consecutive 8
// bytes: a wave's load is 512 contiguous bytes — and the wave's ballot of
// "ineligible" is two finished words, parked in LDS; then thread t writes word t
// of the block: coalesced stores, one word per thread. The grid is (word blocks,
// queries): no [nq, N] intermediate, the tags stay in L2 across queries.
#include "rt_common.h"

namespace rt {
namespace tagf {

constexpr int kThreads = 256;
constexpr int kItems = kThreads * 32;  // per block

__global__ __launch_bounds__(kThreads) void tag_filter_bitmap_kernel(const uint64_t* __restrict__ item_tags,
                                                                    int64_t n_items,
                                                                    const uint64_t* __restrict__ any_of,
                                                                    const uint64_t* __restrict__ none_of,
                                                                    uint32_t* __restrict__ bits, int64_t words,
                                                                    int accumulate) {
    __shared__ uint32_t word[kThreads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.y;
    const uint64_t any = any_of ? any_of[q] : 0ull, none = none_of ? none_of[q] : 0ull;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kItems;
    if (any != 0ull || none != 0ull) {  // block-uniform: no mask filters nothing
#pragma unroll 4
        for (int r = 0; r < 32; ++r) {
            const int64_t p = first + r * kThreads + threadIdx.x;
            bool out = false;  // pad bits stay zero
            if (p < n_items) {
                const uint64_t tg = item_tags[p];
                out = !((any == 0ull || (tg & any) != 0ull) && (tg & none) == 0ull);
            }
            const uint64_t bm = __ballot(out);  // items first + 256 r + 64 wave + [0, 64): two words
            if (lane < 2) word[r * 8 + wave * 2 + lane] = static_cast<uint32_t>(bm >> (32 * lane));
        }
    } else {
        word[threadIdx.x] = 0u;
    }
    __syncthreads();
    const int64_t w = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (w >= words) return;
    uint32_t* const dst = bits + q * words + w;
    *dst = accumulate ? (*dst | word[threadIdx.x]) : word[threadIdx.x];
}

}  // namespace tagf
}  // namespace rt

using namespace rt;

extern "C" int rt_tag_filter_bitmap(const uint64_t* item_tags, int64_t n_items, const uint64_t* any_of,
                                    const uint64_t* none_of, int64_t nq, uint32_t* bits, int64_t words,
                                    int accumulate, void* stream) {
    if (n_items < 0 || nq < 0 || words < (n_items + 31) / 32) return RT_ERR_INVALID;
    if (!item_tags && n_items > 0) return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(item_tags) | reinterpret_cast<uintptr_t>(any_of) |
         reinterpret_cast<uintptr_t>(none_of)) & 7)
        return RT_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(bits) & 3) return RT_ERR_INVALID;
    if (nq == 0 || words == 0) return RT_OK;
    if (!bits) return RT_ERR_INVALID;
    const int64_t blocks = (words + tagf::kThreads - 1) / tagf::kThreads;
    if (blocks > (1ll << 31) - 1) return RT_ERR_UNSUPPORTED;
    for (int64_t q0 = 0; q0 < nq; q0 += 65535) {  // grid.y
        const int64_t n = (nq - q0) < 65535 ? (nq - q0) : 65535;
        hipLaunchKernelGGL(tagf::tag_filter_bitmap_kernel,
                           dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(n)), dim3(tagf::kThreads), 0,
                           as_stream(stream), item_tags, n_items, any_of ? any_of + q0 : nullptr,
                           none_of ? none_of + q0 : nullptr, bits + q0 * words, words, accumulate);
        const int rc = check_launch("tag_filter_bitmap_kernel");
        if (rc) return rc;
    }
    return RT_OK;
}
