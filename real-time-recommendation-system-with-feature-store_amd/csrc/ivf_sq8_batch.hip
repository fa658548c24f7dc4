// IVF-SQ8, list-major batch search (rt_ivf_sq8_topk_batch): rt_ivf_sq8_topk's
// results, bit for bit, with the work grouped by LIST as in rt_ivf_topk_batch
// (ivf_batch.hip). The per-query scan (ivf_sq8.hip) launches a block per (query,
// probed list, chunk): every block streams its list again and converts every
// byte again, and its grid is bound by VALU issue (one v_cvt and one v_fma per
// element per query). Here a byte is converted once per 32 queries and the
// multiply-adds run on the matrix pipe.
//
// Seven launches, all sized by host arguments (no host read, stream-ordered,
// capturable):
//
// 0. sq8_fold (ivf_sq8.hip, as it is): qs[q][j] = q_j step_j and base[q][slot] =
//    bias[q][slot] + b0[q] to the workspace.
// 1-4. ivfb_zero, ivfb_count, ivfb_offsets, ivfb_scatter (ivf_batch_group.h): the
//    (query, probe slot) pairs grouped by list. The plan is rt_ivf_topk_batch's.
// 5. ivf_sq8b_scan: block b = (tile number T = b / chunks, chunk c = b % chunks),
//    the work item of ivfb_scan: (list, tile of 32 pairs naming it, row chunk).
//
//    LDS (157,056 B compiled, one block per CU: the 156,160 B of the four regions
//    below and 896 B of small arrays, the per-slot cnt, thr, qid, qslot and qbase
//    among them):
//      rows   2 x 128 x 144 B =  36,864   codes as BYTES, double-buffered
//      qs     32 x 260 x 4    =  33,280   the tile's folded queries, fp32, whole d
//      cand   32 x 320 x 8    =  81,920   candidate buffers (ivf_batch_group.h)
//      hist   4 x 256 x 4     =   4,096
//    A step stages 128 rows x 8 units of 16 bytes (128 dimensions) — four times
//    the dimensions of ivfb_scan's step in the same row region, because the codes
//    stay bytes. d <= 128: a row tile is ONE step and one barrier, and tile
//    t + 1's global loads (4 uint4 per thread, in registers) are in flight under
//    all 64 MFMAs of tile t. d in (128, 256]: two steps, the second one running
//    only the units inside d. d % 16 == 0 and a unit is 8 k-steps, so no
//    zero-padded k-step is ever issued (a padded step turns a -0.0 sum to +0.0).
//
//    Operand feed of v_mfma_f32_32x32x2_f32, A = the 32 folded queries, B = the
//    wave's 32 rows (wave w owns rows 32 w .. 32 w + 31 of the tile): lane half h
//    needs element 2 s + h of k-step s. At staging a thread de-interleaves its
//    16-byte unit into [8 even bytes | 8 odd bytes] with four v_perm_b32 on the
//    loaded registers and stores it with one ds_write_b128; qs is staged in the
//    same order per unit, [8 even floats | 8 odd floats]. Per unit a lane then
//    issues one ds_read_b64 (its 8 bytes), two ds_read_b128 of qs, 8
//    v_cvt_f32_ubyte0..3 and 8 MFMAs; every lane runs the same instructions.
//    Banks (DESIGN.md §5 has the arithmetic; conflicts were not counted): the row
//    stride is 144 B = 36 words, so a unit's ds_write_b128 of 8 consecutive lanes
//    covers 32 consecutive words of one row and the next row starts 4 banks on;
//    the qs stride of 260 words puts the b128 reads of lanes col .. col + 7 on 32
//    different banks, ivfb_scan's pattern.
//
//    The score: each accumulator starts at its query's base (acc[r] belongs to
//    query tile_row(r, half)), then acc = fmaf(qs[j], (float)code_j, acc), j
//    ascending — one accumulation chain per score, the contract of rtrec_hip.h.
//    Everything behind the score is ivfb_scan's (ivf_batch_group.h).
// 6. flatip_online_finish (topk_online.h, unchanged).
#include "ivf_batch_group.h"
#include "ivf_sq8_fold.h"

namespace rt {
namespace topk {
namespace ivfsq8b {

namespace ib = rt::topk::ivfb;
namespace sq = rt::topk::ivfsq8;

constexpr int kStepUnits = 8;                       // 16-byte units of a row per step: 128 dimensions
constexpr int kRowStride = kStepUnits * 16 + 16;    // 144 B
constexpr int kQS = sq::kMaxD + 4;                  // query stride (floats)
constexpr int kNU = ib::kTileRows * kStepUnits / ib::kThreads;  // units a thread moves per step
constexpr int kBuf = ib::kTileRows * kRowStride;    // one row buffer
static_assert(kNU * ib::kThreads == ib::kTileRows * kStepUnits, "ivf sq8 batch: whole units per thread");

struct Lds {
    static constexpr int kRows = 2 * kBuf;
    static constexpr int kQuery = ib::kQT * kQS * 4;
    static constexpr int kCand = ib::kQT * ib::kCap * static_cast<int>(sizeof(Cand));
    static constexpr int kHist = ib::kWaves * 256 * 4;
    static constexpr int kBytes = kRows + kQuery + kCand + kHist;
    // one block per CU; 1 KiB left for the block's small arrays and the barrier's reduction
    static_assert(kRows == 36864, "ivf sq8 batch: the row region of ivfb_scan");
    static_assert(kBytes + 1024 <= 163840, "ivf sq8 batch: the block's LDS");
};

// bytes b0 .. b15 of a unit -> [b0 b2 .. b14 | b1 b3 .. b15]
__device__ __forceinline__ uint4 deinterleave(uint4 x) {
    uint4 o;
    o.x = __builtin_amdgcn_perm(x.y, x.x, 0x06040200u);
    o.y = __builtin_amdgcn_perm(x.w, x.z, 0x06040200u);
    o.z = __builtin_amdgcn_perm(x.y, x.x, 0x07050301u);
    o.w = __builtin_amdgcn_perm(x.w, x.z, 0x07050301u);
    return o;
}

// four k-steps: the four bytes of `x` against the four floats of `a`
__device__ __forceinline__ void mfma4(f32x16& acc, const float4& a, uint32_t x) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, static_cast<float>(x & 0xFFu), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, static_cast<float>((x >> 8) & 0xFFu), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, static_cast<float>((x >> 16) & 0xFFu), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, static_cast<float>(x >> 24), acc, 0, 0, 0);
}

__global__ __launch_bounds__(ib::kThreads, 1) void ivf_sq8b_scan(
    const float* __restrict__ fold, int stride, const char* __restrict__ codes, int64_t nx, int d, int k,
    const int64_t* __restrict__ list_offsets, int64_t nlist, const int32_t* __restrict__ row_pos, int nprobe,
    int chunks, int64_t rows_per_chunk, const uint32_t* __restrict__ excl, int64_t excl_words,
    uint64_t* __restrict__ partials, const int32_t* __restrict__ pair_start, const int32_t* __restrict__ tile_start,
    const int32_t* __restrict__ pairs, int n_pairs) {
    constexpr int kTileRows = ib::kTileRows, kQT = ib::kQT;
    __shared__ __attribute__((aligned(16))) char lds[Lds::kBytes];
    __shared__ int cnt[kQT];
    __shared__ float thr[kQT];
    __shared__ int qid[kQT], qslot[kQT];
    __shared__ float qbase[kQT];
    char* const rows_l = lds;
    float* const qs = reinterpret_cast<float*>(lds + Lds::kRows);
    Cand* const cand = reinterpret_cast<Cand*>(lds + Lds::kRows + Lds::kQuery);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + Lds::kRows + Lds::kQuery + Lds::kCand) + wave * 256;

    ib::Item w;
    if (!ib::work_item(pair_start, tile_start, n_pairs, chunks, list_offsets, nlist, nullptr, nx, rows_per_chunk, w))
        return;  // block-uniform
    const int64_t row_begin = w.row_begin, row_end = w.row_end;

    const int units = d >> 4;
    const int nsteps = (units + kStepUnits - 1) / kStepUnits;
    const int tiles = static_cast<int>((row_end - row_begin + kTileRows - 1) / kTileRows);
    const int total = tiles * nsteps;

    uint4 R[kNU];
    // step (tile rt, unit group sg): unit f = i * 256 + tid is unit f % 8 of tile row f / 8;
    // a row past the window or a unit past d is staged as zeros and never read as a score
    auto load = [&](int rt, int sg) {
#pragma unroll
        for (int i = 0; i < kNU; ++i) {
            const int f = i * ib::kThreads + tid;
            const int r = f >> 3, u = sg * kStepUnits + (f & 7);
            const int64_t row = row_begin + static_cast<int64_t>(rt) * kTileRows + r;
            R[i] = make_uint4(0u, 0u, 0u, 0u);
            if (row < row_end && u < units) R[i] = *reinterpret_cast<const uint4*>(codes + row * d + u * 16);
        }
    };
    auto store = [&](int b) {
#pragma unroll
        for (int i = 0; i < kNU; ++i) {
            const int f = i * ib::kThreads + tid;
            *reinterpret_cast<uint4*>(rows_l + b * kBuf + (f >> 3) * kRowStride + (f & 7) * 16) = deinterleave(R[i]);
        }
    };

    load(0, 0);
    ib::tile_slots(w, pairs, n_pairs, nprobe, qid, qslot, cnt, thr);
    __syncthreads();
    // the tile's folded queries, per unit [8 even | 8 odd]; an empty slot of the tile: zeros
    for (int idx = tid; idx < kQT * d; idx += ib::kThreads) {
        const int i = idx / d, e = idx - i * d;
        const float v = qid[i] >= 0 ? fold[static_cast<int64_t>(qid[i]) * stride + e] : 0.f;
        const int x = e & 15;
        qs[i * kQS + (e - x) + (x & 1) * 8 + (x >> 1)] = v;
    }
    if (tid < kQT) qbase[tid] = qid[tid] >= 0 ? fold[static_cast<int64_t>(qid[tid]) * stride + d + qslot[tid]] : 0.f;
    store(0);
    __syncthreads();

    f32x16 base;
#pragma unroll
    for (int r = 0; r < 16; ++r) base[r] = qbase[tile_row(r, half)];
    f32x16 acc = base;
    int32_t pos = -1;
    int over = 0;  // decided through the barrier that ends a tile: block-uniform
    int rt = 0, sg = 0;
    for (int stp = 0; stp < total; ++stp) {
        const int b = stp & 1;
        int nrt = rt, nsg = sg + 1;
        if (nsg == nsteps) {
            nsg = 0;
            nrt = rt + 1;
        }
        const bool more = stp + 1 < total;
        if (more) load(nrt, nsg);
        const int64_t row = row_begin + static_cast<int64_t>(rt) * kTileRows + wave * 32 + col;
        // original position of this lane's row: in flight under the scores
        if (sg == 0) pos = row < row_end ? row_pos[row] : -1;
        {
            const float* qa = qs + col * kQS + sg * (kStepUnits * 16) + half * 8;
            const char* xa = rows_l + b * kBuf + (wave * 32 + col) * kRowStride + half * 8;
            const int nu = (units - sg * kStepUnits) < kStepUnits ? (units - sg * kStepUnits) : kStepUnits;
#pragma unroll
            for (int u = 0; u < kStepUnits; ++u) {
                if (u < nu) {  // wave-uniform
                    const uint2 x = *reinterpret_cast<const uint2*>(xa + u * 16);
                    const float4 a0 = *reinterpret_cast<const float4*>(qa + u * 16);
                    const float4 a1 = *reinterpret_cast<const float4*>(qa + u * 16 + 4);
                    mfma4(acc, a0, x.x);
                    mfma4(acc, a1, x.y);
                }
            }
        }
        if (more) store(b ^ 1);
        if (sg + 1 < nsteps) {
            __syncthreads();
        } else {
            const bool valid = row < row_end && pos >= 0 && static_cast<int64_t>(pos) < nx;
            const int mine_over = ib::select_tile(acc, valid, pos, qid, thr, cnt, cand, excl, excl_words);
            acc = base;
            over = __syncthreads_or(mine_over);
            if (over && more) {
                ib::compact_tile_buffers(w.nqt, k, cnt, thr, cand, hist);
                __syncthreads();
            }
        }
        rt = nrt;
        sg = nsg;
    }

    ib::write_tile_lists(w, k, nprobe, chunks, qid, qslot, cnt, cand, hist, partials);
}

}  // namespace ivfsq8b
}  // namespace topk
}  // namespace rt

using namespace rt;
namespace sb = rt::topk::ivfsq8b;
namespace sbi = rt::topk::ivfb;
namespace sbq = rt::topk::ivfsq8;
namespace sbon = rt::topk::online;

// the batch plan's partial lists and tables, then the folded queries [nq][d + nprobe padded to 4] fp32
extern "C" size_t rt_ivf_sq8_topk_batch_workspace_bytes(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows,
                                                        int k, int d) {
    sbi::Plan p;
    if (!sbq::d_ok(d) || !sbi::make_plan(nq, nprobe, nlist, max_list_rows, k, p)) return 256;
    return sbq::align256(sbi::workspace_bytes(nq, nprobe, nlist, k, p)) +
           static_cast<size_t>(nq) * sbq::fold_stride(d, nprobe) * sizeof(float);
}

extern "C" int rt_ivf_sq8_topk_batch(const float* queries, int64_t nq, int d, const uint8_t* codes, int64_t nx,
                                     const float* lo, const float* step, const int64_t* list_offsets, int64_t nlist,
                                     const int32_t* row_pos, const int64_t* probes, const float* bias, int nprobe,
                                     int64_t max_list_rows, int k, const uint32_t* exclude_bits,
                                     int64_t exclude_words, float* out_scores, int64_t* out_ids, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (nq < 0 || nx < 0 || d <= 0 || k <= 0 || nlist <= 0 || nprobe <= 0 || max_list_rows < 0) return RT_ERR_INVALID;
    if (nq == 0) return RT_OK;
    if (!queries || !lo || !step || !out_scores || !out_ids || !list_offsets || !probes ||
        (nx > 0 && (!codes || !row_pos)))
        return RT_ERR_INVALID;
    if (k > sbi::kMaxK || nprobe > sbi::kMaxProbe) return RT_ERR_UNSUPPORTED;
    if (!sbq::d_ok(d)) return RT_ERR_UNSUPPORTED;
    if (nx >= 0x7FFFFFFFll) return RT_ERR_UNSUPPORTED;  // positions are int32
    sbi::Plan p;
    if (!sbi::make_plan(nq, nprobe, nlist, max_list_rows, k, p)) return RT_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(step) |
         reinterpret_cast<uintptr_t>(codes)) & 15)
        return RT_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(bias) & 3) || (exclude_bits && exclude_words < (nx + 31) / 32))
        return RT_ERR_INVALID;
    const size_t tables = sbq::align256(sbi::workspace_bytes(nq, nprobe, nlist, k, p));
    const int stride = sbq::fold_stride(d, nprobe);
    if (!workspace || workspace_bytes < tables + static_cast<size_t>(nq) * stride * sizeof(float))
        return RT_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return RT_ERR_INVALID;

    hipStream_t st = as_stream(stream);
    const int64_t pairs = nq * nprobe;
    const sbi::Tables t = sbi::carve(workspace, nq, nprobe, nlist, k, p);
    float* const fold = reinterpret_cast<float*>(static_cast<char*>(workspace) + tables);
    const int stages = sbi::stages();
    int rc = RT_OK;
    if (stages & 1) {  // the fold belongs to the grouping bit
        rc = sbq::launch_fold(queries, nq, d, lo, step, bias, nprobe, stride, fold, st);
        if (rc) return rc;
        rc = sbi::launch_grouping(t, probes, pairs, nlist, st);
        if (rc) return rc;
    }
    if (stages & 2) {
        hipLaunchKernelGGL(sb::ivf_sq8b_scan, dim3(static_cast<unsigned>(p.blocks)), dim3(sbi::kThreads), 0, st, fold,
                           stride, reinterpret_cast<const char*>(codes), nx, d, k, list_offsets, nlist, row_pos,
                           nprobe, p.chunks, p.rows_per_chunk, exclude_bits, exclude_words, t.partials, t.pair_start,
                           t.tile_start, t.pair_of, static_cast<int>(pairs));
        rc = check_launch("ivf_sq8b_scan");
        if (rc) return rc;
    }
    if (!(stages & 4)) return RT_OK;
    return sbon::launch_finish(t.partials, nprobe * p.chunks, k, out_scores, out_ids, 0, nq, st);
}
