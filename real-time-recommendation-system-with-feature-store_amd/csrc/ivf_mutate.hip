// In-place mutation of IVF lists stored with slack (rt_ivf_lists_update): the
// streaming item_update path of the reference (-> RetrievalEngine.update_index,
// src/serving/retrieval.py:228-246, 629-641) on its default "IVF1024,Flat"
// index. A batch of m operations (position, new list or -1, new row) overwrites
// rows where they lie, moves rows between lists and withdraws rows, in O(batch)
// plus one pass over the 4-byte row_pos entries of the lists that lose rows.
//
// Layout (rtrec_hip.h): list l owns the stored rows [off[l], off[l + 1]) — its
// capacity; its live rows are the first list_len[l] of them and every slot
// behind them holds row_pos = -1. pos_slot / assign map a position to its
// stored row and its list (-1: the position has no row).
//
// Three launches after a memset of the status pair; the kernel boundaries are
// the only ordering between workgroups (no hand-off, no wait loop):
//   prepare  one thread per operation: checks it (position inside the capacity,
//            new_list in [-1, nlist), the position's stored row consistent with
//            row_pos / list_offsets), records the operation's CURRENT list and
//            slot in the workspace — the apply then never reads a pos_slot /
//            assign entry that another workgroup writes — and counts refused
//            operations in status[1];
//   count    one workgroup per list: entries (new_list == l), leavers and
//            joiners of the list; a list whose new length exceeds its capacity
//            adds one to status[0];
//   apply    one workgroup per list, and nothing at all when either status word
//            is set. Placement rule (deterministic: the state and the batch fix
//            every byte):
//              * a position whose list does not change is overwritten in place;
//              * holes = the slots of the list's leavers in ascending slot
//                order, joiners in ascending operation order: joiner j takes
//                hole j, surplus joiners append at len, len + 1, ...;
//              * surplus holes below the new length take the surviving rows at
//                or past the new length, both in ascending slot order (sources
//                >= new length > destinations: the moves do not alias);
//              * every slot at or past the new length ends with row_pos = -1.
//            A position entry (pos_slot, assign) has one writer: the workgroup
//            of the list it joins, or of the list it leaves when it joins none.
// Rows move as 16-byte vectors, lanes flattened over (row, 16-B chunk).
#include "topk_online.h"

namespace rt {
namespace ivfm {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / RT_WAVE;

// workspace: int32 arrays, in this order
struct Ws {
    int32_t* old_list;   // [m] the operation's current list (-1: no row)
    int32_t* old_slot;   // [m] its current stored row
    int32_t* ent;        // [m] per list, ascending: the operations with new_list == l
    int32_t* jrank;      // [m] beside ent: rank among the list's joiners, -1 for an overwrite
    int32_t* hole;       // [m] per list, ascending: the list-local slots its leavers free
    int32_t* cnt_new;    // [nlist]
    int32_t* cnt_leave;  // [nlist]
    int32_t* cnt_join;   // [nlist]
};

inline size_t ws_bytes(int64_t nlist, int64_t m) {
    const size_t words = 5 * static_cast<size_t>(m) + 3 * static_cast<size_t>(nlist);
    return (words * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
}

inline Ws ws_layout(void* base, int64_t nlist, int64_t m) {
    int32_t* p = static_cast<int32_t*>(base);
    Ws w;
    w.old_list = p;
    w.old_slot = p + m;
    w.ent = p + 2 * m;
    w.jrank = p + 3 * m;
    w.hole = p + 4 * m;
    w.cnt_new = p + 5 * m;
    w.cnt_leave = w.cnt_new + nlist;
    w.cnt_join = w.cnt_leave + nlist;
    return w;
}

__global__ __launch_bounds__(kThreads) void prepare_kernel(const int64_t* __restrict__ list_offsets, int64_t nlist,
                                                           const int32_t* __restrict__ row_pos,
                                                           const int32_t* __restrict__ pos_slot,
                                                           const int64_t* __restrict__ assign, int64_t total_rows,
                                                           const int64_t* __restrict__ positions,
                                                           const int64_t* __restrict__ new_list, int64_t m, Ws ws,
                                                           int32_t* __restrict__ status) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= m) return;
    const int64_t p = positions[i], nl = new_list[i];
    int32_t ol = -1, os = -1;
    bool ok = p >= 0 && p < total_rows && nl >= -1 && nl < nlist;
    if (ok) {
        const int32_t s = pos_slot[p];
        if (s >= 0) {  // the position has a row: it must be the one the lists name
            const int64_t a = assign[p];
            ok = a >= 0 && a < nlist && s < total_rows;
            if (ok) ok = s >= list_offsets[a] && s < list_offsets[a + 1] && row_pos[s] == static_cast<int32_t>(p);
            if (ok) {
                ol = static_cast<int32_t>(a);
                os = s;
            }
        }
    }
    ws.old_list[i] = ol;
    ws.old_slot[i] = os;
    if (!ok) atomicAdd(status + 1, 1);
}

// list l as the apply sees it: offset, capacity and live length, clamped to the stored rows
struct ListRange {
    int64_t off;
    int32_t cap, len;
};

__device__ __forceinline__ ListRange list_range(const int64_t* __restrict__ list_offsets,
                                                const int64_t* __restrict__ list_len, int64_t l, int64_t total_rows) {
    int64_t lo = list_offsets[l], hi = list_offsets[l + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > total_rows ? total_rows : hi;
    ListRange r;
    r.off = lo;
    r.cap = hi > lo ? static_cast<int32_t>(hi - lo) : 0;
    const int64_t n = list_len[l];
    r.len = n < 0 ? 0 : (n > r.cap ? r.cap : static_cast<int32_t>(n));
    return r;
}

__device__ __forceinline__ int block_sum(int v, int* s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RT_WAVE);
    const int lane = threadIdx.x & (RT_WAVE - 1), wave = threadIdx.x / RT_WAVE;
    __syncthreads();  // s_w may still be read from the call before
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += s_w[w];
    return t;
}

// rank of this thread among the block's threads with `f`, in thread order; total = their number
__device__ __forceinline__ int block_rank(bool f, int* s_w, int& total) {
    const int lane = threadIdx.x & (RT_WAVE - 1), wave = threadIdx.x / RT_WAVE;
    const unsigned long long b = __ballot(f);
    const int r = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // s_w may still be read from the call before
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) base += s_w[w];
        total += s_w[w];
    }
    return base + r;
}

__global__ __launch_bounds__(kThreads) void count_kernel(const int64_t* __restrict__ list_offsets, int64_t nlist,
                                                         const int64_t* __restrict__ list_len, int64_t total_rows,
                                                         const int64_t* __restrict__ new_list, int64_t m, Ws ws,
                                                         int32_t* __restrict__ status) {
    __shared__ int s_w[kWaves];
    const int64_t l = blockIdx.x;
    int c_new = 0, c_leave = 0, c_join = 0;
    for (int64_t i = threadIdx.x; i < m; i += kThreads) {
        const bool is_new = new_list[i] == l, was = ws.old_list[i] == l;
        c_new += is_new;
        c_leave += was && !is_new;
        c_join += is_new && !was;
    }
    c_new = block_sum(c_new, s_w);
    c_leave = block_sum(c_leave, s_w);
    c_join = block_sum(c_join, s_w);
    if (threadIdx.x == 0) {
        ws.cnt_new[l] = c_new;
        ws.cnt_leave[l] = c_leave;
        ws.cnt_join[l] = c_join;
        const ListRange r = list_range(list_offsets, list_len, l, total_rows);
        if (static_cast<int64_t>(r.len) - c_leave + c_join > r.cap) atomicAdd(status, 1);
    }
}

__global__ __launch_bounds__(kThreads) void apply_kernel(u32x4* __restrict__ rows, int64_t total_rows, int vpr,
                                                         const int64_t* __restrict__ list_offsets, int64_t nlist,
                                                         int64_t* __restrict__ list_len, int32_t* __restrict__ row_pos,
                                                         int32_t* __restrict__ pos_slot, int64_t* __restrict__ assign,
                                                         const int64_t* __restrict__ positions,
                                                         const int64_t* __restrict__ new_list,
                                                         const u32x4* __restrict__ new_rows, int64_t m, Ws ws,
                                                         const int32_t* __restrict__ status) {
    __shared__ int s_w[kWaves];
    __shared__ int s_src[kThreads], s_dst[kThreads];
    if (status[0] != 0 || status[1] != 0) return;  // all or nothing (grid-uniform)
    const int64_t l = blockIdx.x;
    const int tid = threadIdx.x;
    const int n_new = ws.cnt_new[l], n_leave = ws.cnt_leave[l], n_join = ws.cnt_join[l];
    if (n_new == 0 && n_leave == 0) return;  // block-uniform: the list is not touched
    const ListRange lr = list_range(list_offsets, list_len, l, total_rows);
    const int64_t off = lr.off;
    const int len = lr.len, cap = lr.cap;

    // where the list's entries and holes start in the workspace
    int64_t be = 0, bh = 0;
    {
        int a = 0, b = 0;  // each sum <= m < 2^31
        for (int64_t j = tid; j < l; j += kThreads) {
            a += ws.cnt_new[j];
            b += ws.cnt_leave[j];
        }
        be = block_sum(a, s_w);
        bh = block_sum(b, s_w);
    }

    // A. the operations in ascending order: leavers free their slot, entries are listed
    int e_run = 0, j_run = 0;
    for (int64_t c0 = 0; c0 < m; c0 += kThreads) {
        const int64_t i = c0 + tid;
        bool is_new = false, was = false;
        int64_t nl = -1;
        if (i < m) {
            nl = new_list[i];
            is_new = nl == l;
            was = ws.old_list[i] == l;
        }
        if (!__syncthreads_or(is_new || was)) continue;  // block-uniform
        const bool is_join = is_new && !was;
        if (was && !is_new) {
            row_pos[ws.old_slot[i]] = -1;
            if (nl < 0) {  // joins no list: this workgroup is the entry's writer
                const int64_t p = positions[i];
                pos_slot[p] = -1;
                assign[p] = -1;
            }
        }
        int te, tj;
        const int re = block_rank(is_new, s_w, te);
        const int rj = block_rank(is_join, s_w, tj);
        if (is_new && e_run + re < n_new) {
            ws.ent[be + e_run + re] = static_cast<int32_t>(i);
            ws.jrank[be + e_run + re] = is_join ? j_run + rj : -1;
        }
        e_run += te;
        j_run += tj;
    }
    const int n_ent = e_run < n_new ? e_run : n_new;
    __syncthreads();

    // B. the holes in ascending slot order
    int n_hole = 0;
    if (n_leave > 0) {
        for (int s0 = 0; s0 < len; s0 += kThreads) {
            const int s = s0 + tid;
            const bool f = s < len && row_pos[off + s] == -1;
            int t;
            const int r = block_rank(f, s_w, t);
            if (f && n_hole + r < n_leave) ws.hole[bh + n_hole + r] = s;
            n_hole += t;
        }
        if (n_hole > n_leave) n_hole = n_leave;
        __syncthreads();
    }

    // C. overwrites and joiners: (entry, 16-byte chunk) over the threads
    for (int64_t e = tid; e < static_cast<int64_t>(n_ent) * vpr; e += kThreads) {
        const int x = static_cast<int>(e / vpr), c = static_cast<int>(e - static_cast<int64_t>(x) * vpr);
        const int i = ws.ent[be + x], jr = ws.jrank[be + x];
        int64_t dst;
        if (jr < 0) {
            dst = ws.old_slot[i];
        } else {
            int d;
            if (jr < n_leave) {
                if (jr >= n_hole) continue;  // positions were not unique: fewer holes than leavers
                d = ws.hole[bh + jr];
            } else {
                d = len + (jr - n_leave);
            }
            if (d < 0 || d >= cap) continue;
            dst = off + d;
            if (c == 0) {
                const int64_t p = positions[i];
                row_pos[dst] = static_cast<int32_t>(p);
                pos_slot[p] = static_cast<int32_t>(dst);
                assign[p] = l;
            }
        }
        rows[dst * vpr + c] = new_rows[static_cast<int64_t>(i) * vpr + c];
    }

    // D. surplus holes below the new length take the surviving tail
    int new_len = len - n_leave + n_join;
    new_len = new_len < 0 ? 0 : (new_len > cap ? cap : new_len);
    if (n_leave > n_join) {
        __syncthreads();  // an overwritten row (C) may be one that moves
        int t_run = 0;
        for (int s0 = new_len; s0 < len; s0 += kThreads) {
            const int s = s0 + tid;
            const int32_t p = s < len ? row_pos[off + s] : -1;
            int t;
            const int r = block_rank(p >= 0, s_w, t);
            const int h = n_join + t_run + r;
            int d = -1;
            if (p >= 0 && h < n_hole) d = ws.hole[bh + h];
            const bool mv = d >= 0 && d < new_len;
            if (p >= 0) {  // ranks 0 .. t - 1: every pair the copy below reads is written
                s_src[r] = mv ? s : -1;
                s_dst[r] = d;
                if (mv) {
                    row_pos[off + d] = p;
                    pos_slot[p] = static_cast<int32_t>(off + d);
                    row_pos[off + s] = -1;
                }
            }
            __syncthreads();
            for (int e = tid; e < t * vpr; e += kThreads) {
                const int x = e / vpr, c = e - x * vpr;
                if (s_src[x] >= 0) rows[(off + s_dst[x]) * vpr + c] = rows[(off + s_src[x]) * vpr + c];
            }
            __syncthreads();
            t_run += t;
        }
    }
    if (tid == 0) list_len[l] = new_len;
}

}  // namespace ivfm
}  // namespace rt

using namespace rt;
namespace ivm = rt::ivfm;

extern "C" size_t rt_ivf_lists_update_workspace_bytes(int64_t nlist, int64_t m) {
    return ivm::ws_bytes(nlist < 0 ? 0 : nlist, m < 0 ? 0 : m);
}

extern "C" int rt_ivf_lists_update(void* rows, int64_t total_rows, int d, int dtype, const int64_t* list_offsets,
                                   int64_t nlist, int64_t* list_len, int32_t* row_pos, int32_t* pos_slot,
                                   int64_t* assign, const int64_t* positions, const int64_t* new_list,
                                   const void* new_rows, int64_t m, int32_t* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (total_rows < 0 || m < 0 || nlist <= 0 || d <= 0) return RT_ERR_INVALID;
    if (dtype != RT_F32 && dtype != RT_F16 && dtype != RT_BF16) return RT_ERR_INVALID;
    if (!rt::topk::online::shape_ok(d, dtype)) return RT_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(new_rows)) & 15) return RT_ERR_INVALID;
    if (m == 0) return RT_OK;
    if (!rows || !list_offsets || !list_len || !row_pos || !pos_slot || !assign || !positions || !new_list ||
        !new_rows || !status)
        return RT_ERR_INVALID;
    // slots and operation indices are int32
    if (total_rows >= 0x7FFFFFFFll || m >= 0x7FFFFFFFll || nlist >= 0x7FFFFFFFll) return RT_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ivm::ws_bytes(nlist, m)) return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return RT_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const ivm::Ws ws = ivm::ws_layout(workspace, nlist, m);
    const int vpr = d * (dtype == RT_F32 ? 4 : 2) / 16;
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) {
        set_last_error("ivf_lists_update status memset", e);
        return RT_ERR_HIP;
    }
    hipLaunchKernelGGL(ivm::prepare_kernel, dim3(static_cast<unsigned>((m + ivm::kThreads - 1) / ivm::kThreads)),
                       dim3(ivm::kThreads), 0, st, list_offsets, nlist, row_pos, pos_slot, assign, total_rows,
                       positions, new_list, m, ws, status);
    int rc = check_launch("ivf_lists_prepare");
    if (rc) return rc;
    hipLaunchKernelGGL(ivm::count_kernel, dim3(static_cast<unsigned>(nlist)), dim3(ivm::kThreads), 0, st,
                       list_offsets, nlist, list_len, total_rows, new_list, m, ws, status);
    rc = check_launch("ivf_lists_count");
    if (rc) return rc;
    hipLaunchKernelGGL(ivm::apply_kernel, dim3(static_cast<unsigned>(nlist)), dim3(ivm::kThreads), 0, st,
                       static_cast<ivm::u32x4*>(rows), total_rows, vpr, list_offsets, nlist, list_len, row_pos,
                       pos_slot, assign, positions, new_list, static_cast<const ivm::u32x4*>(new_rows), m, ws, status);
    return check_launch("ivf_lists_apply");
}
