// C ABI of the online (small-batch) Flat-IP top-K: rt_flatip_topk_online,
// rt_flatip_topk_online_lists, rt_flatip_topk_online_tags, their plan and
// workspace queries. The kernels
// and their launchers live in topk_online.h, which csrc/ivf.hip shares.
#include "topk_online.h"

using namespace rt;
namespace on = rt::topk::online;

static_assert(RT_ONLINE_MAX_NQ == on::kMaxNq && RT_ONLINE_MAX_K == on::kMaxK, "rtrec_hip.h restates the kernel's limits");

extern "C" int rt_flatip_topk_online_plan(int64_t nq, int64_t nx, int d, int dtype, int k, int64_t* out) {
    if (nq <= 0 || nx < 0 || d <= 0 || k <= 0 || !out) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (nq > on::kMaxNq || k > on::kMaxK || !on::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    const on::OnlinePlan p = on::make_plan(nx);
    out[0] = p.blocks;
    out[1] = p.rows_per_block;
    return RT_OK;
}

extern "C" size_t rt_flatip_topk_online_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k) {
    int64_t plan[2];
    if (rt_flatip_topk_online_plan(nq, nx, d, dtype, k, plan) != RT_OK) return 256;
    const size_t need = on::workspace_bytes(nq, k, on::make_plan(nx));
    return need < 256 ? 256 : need;
}

static_assert(RT_ONLINE_MAX_EXCL_SOURCES == on::kMaxSrc, "rtrec_hip.h restates the kernel's limits");

// the entry points: the dense bitmap (la == nullptr) or the lists; tags != nullptr:
// the tag filter on top of the lists (la != nullptr then, with any number of sources)
static int online_search(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype, int k,
                         const uint32_t* exclude_bits, int64_t exclude_words, const on::ListArgs<true>* la,
                         const on::TagSrc* tags, int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !out_scores || !out_ids || (nx > 0 && !items)) return RT_ERR_INVALID;
    if (nq > on::kMaxNq || k > on::kMaxK) return RT_ERR_UNSUPPORTED;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!on::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0xFFFFFFFFll || (id_offset + nx) >= 0xFFFFFFFFll || id_offset < 0) return RT_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(items)) & 15) return RT_ERR_INVALID;
    if (exclude_bits && exclude_words < (nx + 31) / 32) return RT_ERR_INVALID;
    if (!workspace || workspace_bytes < rt_flatip_topk_online_workspace_bytes(nq, nx, d, dtype, k))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return RT_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const on::OnlinePlan p = on::make_plan(nx);
    uint64_t* partials = static_cast<uint64_t*>(workspace);
    int blocks = 0;  // empty corpus: the finish alone, every slot (-FLT_MAX, -1)
    if (nx > 0) {
        int rc;
        const int n = static_cast<int>(nq);
        if (tags) {
            on::TagArgs<true> ta;
            static_cast<on::TagSrc&>(ta) = *tags;
            switch (dtype) {
                case RT_F32: rc = on::launch_scan<float, true, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la, ta); break;
                case RT_F16: rc = on::launch_scan<__half, true, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la, ta); break;
                default: rc = on::launch_scan<__hip_bfloat16, true, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la, ta); break;
            }
        } else if (la) {
            switch (dtype) {
                case RT_F32: rc = on::launch_scan<float, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la); break;
                case RT_F16: rc = on::launch_scan<__half, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la); break;
                default: rc = on::launch_scan<__hip_bfloat16, true>(queries, n, items, nx, d, k, nullptr, 0, p, partials, st, *la); break;
            }
        } else {
            switch (dtype) {
                case RT_F32: rc = on::launch_scan<float>(queries, n, items, nx, d, k, exclude_bits, exclude_words, p, partials, st); break;
                case RT_F16: rc = on::launch_scan<__half>(queries, n, items, nx, d, k, exclude_bits, exclude_words, p, partials, st); break;
                default: rc = on::launch_scan<__hip_bfloat16>(queries, n, items, nx, d, k, exclude_bits, exclude_words, p, partials, st); break;
            }
        }
        if (rc) return rc;
        blocks = p.blocks;
    }
    return on::launch_finish(partials, blocks, k, out_scores, out_ids, id_offset, nq, st);
}

extern "C" int rt_flatip_topk_online(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                                     int dtype, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                                     int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return online_search(queries, nq, items, nx, d, dtype, k, exclude_bits, exclude_words, nullptr, nullptr, id_offset,
                         out_scores, out_ids, workspace, workspace_bytes, stream);
}

// the lists entry points: `filter` is null for rt_flatip_topk_online_lists
static int online_search_lists(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                               int k, const RtExclusionLists* lists, int n_lists, const RtTagFilter* filter,
                               int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                               size_t workspace_bytes, void* stream) {
    on::TagSrc tags{};
    if (filter) {
        if (!filter->item_tags && nx > 0) return RT_ERR_INVALID;
        if ((reinterpret_cast<uintptr_t>(filter->item_tags) | reinterpret_cast<uintptr_t>(filter->any_of) |
             reinterpret_cast<uintptr_t>(filter->none_of)) & 7)
            return RT_ERR_INVALID;
        tags = on::TagSrc{filter->item_tags, filter->any_of, filter->none_of};
    }
    if (n_lists < 0 || (n_lists > 0 && !lists)) return RT_ERR_INVALID;
    if (n_lists > RT_ONLINE_MAX_EXCL_SOURCES) return RT_ERR_UNSUPPORTED;
    on::ListArgs<true> la{};
    la.n = n_lists;
    for (int s = 0; s < n_lists; ++s) {
        const RtExclusionLists& L = lists[s];
        if (!L.offsets || L.n_rows < 0 || (L.n_rows > 0 && !L.items)) return RT_ERR_INVALID;
        la.src[s] = on::ListSrc{L.offsets, L.items, L.rows, L.n_rows};
    }
    // no source and no filter: the plain scan, bit for bit rt_flatip_topk_online without a bitmap
    return online_search(queries, nq, items, nx, d, dtype, k, nullptr, 0, (n_lists || filter) ? &la : nullptr,
                         filter ? &tags : nullptr, id_offset, out_scores, out_ids, workspace, workspace_bytes, stream);
}

extern "C" int rt_flatip_topk_online_lists(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                                           int dtype, int k, const RtExclusionLists* lists, int n_lists,
                                           int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    return online_search_lists(queries, nq, items, nx, d, dtype, k, lists, n_lists, nullptr, id_offset, out_scores,
                               out_ids, workspace, workspace_bytes, stream);
}

extern "C" int rt_flatip_topk_online_tags(const void* queries, int64_t nq, const void* items, int64_t nx, int d,
                                          int dtype, int k, const RtExclusionLists* lists, int n_lists,
                                          const RtTagFilter* filter, int64_t id_offset, float* out_scores,
                                          int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    return online_search_lists(queries, nq, items, nx, d, dtype, k, lists, n_lists, filter, id_offset, out_scores,
                               out_ids, workspace, workspace_bytes, stream);
}
