/*
 * rtrec_hip.h — C ABI of the MI355X (gfx950) two-tower retrieval hot path.
 *
 * One shared library, librtrec_hip.so, built with hipcc --offload-arch=gfx950.
 * Conventions (all entry points):
 *   - plain device pointers and sizes, no framework types;
 *   - `stream` is a hipStream_t passed as void* (0 = null stream); every call
 *     is stream-ordered, never synchronises, never allocates (caller-owned
 *     workspaces), so calls are capturable in a hipGraph;
 *   - return RT_OK (0) or a negative rt_status; no C++ exception crosses the ABI;
 *   - row-major contiguous matrices unless a leading dimension is given.
 * Each entry names the reference interface it replaces (paths relative to the
 * reference repo yxyxcyx/Real-Time-Recommendation-System-with-Feature-Store).
 */
#ifndef RTREC_HIP_H
#define RTREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,     /* bad argument (null pointer, size, alignment)       */
    RT_ERR_UNSUPPORTED = -2, /* valid but not implemented shape/dtype/k            */
    RT_ERR_WORKSPACE = -3,   /* workspace too small (query *_workspace_bytes)      */
    RT_ERR_HIP = -4          /* a HIP launch/runtime call failed                    */
} rt_status;

typedef enum { RT_F32 = 0, RT_F16 = 1, RT_BF16 = 2 } rt_dtype;

typedef enum {
    RT_ACT_RELU = 0,       /* nn.ReLU            (src/models/two_tower.py:80) */
    RT_ACT_GELU = 1,       /* nn.GELU (erf)      (:81)                         */
    RT_ACT_LEAKY_RELU = 2, /* nn.LeakyReLU(0.1)  (:82)                         */
    RT_ACT_TANH = 3,       /* nn.Tanh            (:83)                         */
    RT_ACT_SIGMOID = 4,    /* nn.Sigmoid         (:84)                         */
    RT_ACT_NONE = 5
} rt_act;

int rt_abi_version(void);
const char* rt_status_string(int status);
/* last HIP error string recorded by a failing call (thread-local) */
const char* rt_last_error(void);

/* ------------------------------------------------------------------------
 * Row gather (HBM-bound).
 * Replaces: numpy fancy indexing `self.user_features[user_idx]`,
 * `self.movie_features[pos_item_idx]`, `self.movie_features[neg_item_indices]`
 * (src/training/datasets/movielens.py:108-116) and the `nn.Embedding` lookup
 * (src/models/two_tower.py:115-119, 257-261).
 * out[r] = table[ids[r] - row_begin] for ids in [row_begin, row_begin+n_rows);
 * other ids produce a zero row and are counted in *oob_count (may be NULL).
 * A sharded table passes its first global row as row_begin.
 * row_bytes: multiple of 4; table/out 4-byte aligned (16 B for the wide path).
 * ------------------------------------------------------------------------ */
int rt_gather_rows(const void* table, int64_t row_begin, int64_t n_rows, int64_t row_bytes,
                   const int64_t* ids, int64_t n_ids, void* out, int32_t* oob_count, void* stream);

/* nn.Embedding backward (padding_idx rows receive no gradient):
 * grad_table[ids[r]] += grad_out[r] for ids != padding_idx (fp32 atomics). */
int rt_scatter_add_rows_f32(float* grad_table, int64_t n_rows, int dim, const int64_t* ids,
                            int64_t n_ids, const float* grad_out, int64_t padding_idx, void* stream);

/* ------------------------------------------------------------------------
 * In-place row overwrite and order-preserving row removal of a dense corpus.
 * Replaces: FaissIndex.update / FaissIndex.remove, which on a Flat index only
 * log "Flat index doesn't support direct updates / removal. Consider periodic
 * rebuilds." (src/serving/retrieval.py:228-246), so that the streaming
 * item_update path (RetrievalEngine.update_index, :629-641) appends a changed
 * item a second time and a withdrawn item never leaves.
 * Both: row_bytes % 16 == 0, row pointers 16-byte aligned (RT_ERR_INVALID
 * otherwise; every stored row width of the index qualifies), row_bytes <= 2^24
 * (RT_ERR_UNSUPPORTED above).
 *
 * rt_scatter_rows: dst[positions[i]] = src[i], i < n. A position outside
 *   [0, dst_rows) is skipped and counted in *oob_count (may be NULL).
 *   POSITIONS MUST BE UNIQUE (the caller guarantees it): two rows scattered to
 *   one position leave that row a mix of both. n == 0: RT_OK, no launch.
 *
 * rt_rows_compact: stable stream compaction, out of place. Row r < n_rows is
 *   kept iff bit r % 32 of keep_bits[r / 32] is set (bits of the last word
 *   beyond n_rows are ignored). Kept rows land in dst[0 .. *n_kept) in source
 *   order, as faiss.IndexFlat.remove_ids shifts later rows down; dst rows at
 *   and beyond *n_kept are not written; src is not written. n_kept is a DEVICE
 *   int64, always written (n_rows == 0 writes 0; with n_rows == 0 it may be
 *   NULL and the call is then host-only). No host read: stream-ordered and
 *   capturable. Two launches (segment offsets by one workgroup, then the move),
 *   no cross-workgroup hand-off.
 *   RT_ERR_INVALID: dst_rows < n_rows (the host side does not know the count,
 *   so the safe bound is the contract); [src, src + n_rows*row_bytes) and
 *   [dst, dst + dst_rows*row_bytes) overlapping; keep_words < ceil(n_rows/32);
 *   workspace_bytes < rt_rows_compact_workspace_bytes(n_rows); a workspace
 *   that is NULL or not 8-byte aligned.
 * ------------------------------------------------------------------------ */
int rt_scatter_rows(const void* src, int64_t n, int64_t row_bytes, const int64_t* positions,
                    void* dst, int64_t dst_rows, int32_t* oob_count, void* stream);
size_t rt_rows_compact_workspace_bytes(int64_t n_rows);
int rt_rows_compact(const void* src, int64_t n_rows, int64_t row_bytes,
                    const uint32_t* keep_bits, int64_t keep_words,
                    void* dst, int64_t dst_rows, int64_t* n_kept,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * faiss.normalize_L2 (src/serving/retrieval.py:86,167,214), in place:
 * x[i] *= 1/sqrtf(sum_j x[i][j]^2) when the sum is > 0. The sum is a
 * sequential fmaf chain over j (the order oracle/flatip.c defines).
 * ------------------------------------------------------------------------ */
int rt_l2_renorm_f32(float* x, int64_t n, int d, void* stream);

/* ------------------------------------------------------------------------
 * Brute-force inner-product top-K (faiss.IndexFlatIP.search,
 * src/serving/retrieval.py:96-98,171; and the masked np.dot + argsort of
 * scripts/evaluate_model.py:217-232).
 * queries [nq, d], items [nx, d], both `dtype`, rows 16-byte aligned:
 * f32: d % 4 == 0, d <= 256; f16/bf16: d % 8 == 0, d <= 256; 1 <= k <= 512;
 * nx + id_offset < 2^32 - 1.
 * exclude_bits: optional uint32 bitmap [nq, exclude_words]; bit j of row q set
 *   means item j is skipped for query q.
 * Result rows: the first k of the (score desc, id asc) order (lower id wins
 * exact ties, as Faiss's strict heap insertion does); out_ids = item index +
 * id_offset; unfilled slots (k > eligible items) = (-FLT_MAX, -1).
 * fp32 scores are a sequential fmaf chain over d (bit-identical to the oracle).
 * ------------------------------------------------------------------------ */
size_t rt_flatip_topk_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k);
int rt_flatip_topk(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                   int k, const uint32_t* exclude_bits, int64_t exclude_words, int64_t id_offset,
                   float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Online (small-batch) search: the same contract as rt_flatip_topk — same
 * arguments, same result rows, fp32 scores bit-identical to the oracle, and
 * f16/bf16 scores the same fp32 fmaf chain over the widened elements — for
 * 1 <= nq <= RT_ONLINE_MAX_NQ and k <= RT_ONLINE_MAX_K, bound by one streaming
 * pass over the corpus instead of by query tiles. Serves the reference's
 * per-request path: faiss.IndexFlatIP.search with ONE user embedding
 * (src/serving/retrieval.py:141-197 at Q = 1, called from
 * src/serving/service.py:268-302). Two launches (a scan whose grid is sized by
 * rows, one finish block per query), stream-ordered, capturable.
 *   rt_flatip_topk_online: RT_ERR_UNSUPPORTED for nq > RT_ONLINE_MAX_NQ or
 *     k > RT_ONLINE_MAX_K (and for the d / dtype / id range rt_flatip_topk
 *     refuses); RT_ERR_INVALID and RT_ERR_WORKSPACE as rt_flatip_topk;
 *     nx == 0: every slot (-FLT_MAX, -1). The workspace is 8-byte aligned.
 *   rt_flatip_topk_online_workspace_bytes: the per-block partial lists
 *     [nq][k][blocks] of 8-byte composite keys (256 for a refused shape).
 *   rt_flatip_topk_online_plan: host only, no device work: out = {blocks,
 *     rows_per_block} of the scan (block b owns the contiguous rows
 *     [b * rows_per_block, min(nx, (b + 1) * rows_per_block))). */
#define RT_ONLINE_MAX_NQ 8
#define RT_ONLINE_MAX_K 128
size_t rt_flatip_topk_online_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k);
int rt_flatip_topk_online_plan(int64_t nq, int64_t nx, int d, int dtype, int k, int64_t* out);
int rt_flatip_topk_online(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                          int k, const uint32_t* exclude_bits, int64_t exclude_words, int64_t id_offset,
                          float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Online search with exclusion LISTS: rt_flatip_topk_online with the dense
 * bitmap replaced by up to RT_ONLINE_MAX_EXCL_SOURCES CSR sources that the
 * scan reads itself (the request schema's exclude_items, src/api/schemas.py:
 * 31-34, and the evaluator's per-user train items, src/evaluation/metrics.py:
 * 252-282, for the serving path): no bitmap in HBM, no launch to fill one.
 *   A source: device CSR `offsets` [n_rows + 1] / `items`; query q uses CSR row
 *   rows ? rows[q] : q (`rows`: device, [nq]); a row outside [0, n_rows) = no
 *   exclusions — the row convention of rt_exclusion_bitmap. Items are LOCAL
 *   corpus positions (before id_offset, as bit j of the bitmap is), ascending
 *   within a CSR row; duplicates are allowed, items >= nx are ignored. A row
 *   that does not ascend gives unspecified exclusions for that query, nothing
 *   worse. Query q skips the union of its rows in all sources. Any list
 *   length: a list may exclude every row (then every slot is (-FLT_MAX, -1)).
 *   n_lists == 0: rt_flatip_topk_online without a bitmap, bit for bit.
 *   Result rows, workspace (rt_flatip_topk_online_workspace_bytes) and plan
 *   (rt_flatip_topk_online_plan) are rt_flatip_topk_online's.
 *   Status, before any device work: RT_ERR_INVALID for n_lists < 0, lists ==
 *   NULL with n_lists > 0, a source with offsets == NULL, n_rows < 0, or items
 *   == NULL with n_rows > 0; RT_ERR_UNSUPPORTED for n_lists >
 *   RT_ONLINE_MAX_EXCL_SOURCES; then every refusal of rt_flatip_topk_online.
 *   The batch kernel rt_flatip_topk keeps the bitmap operand. */
typedef struct {
    const int64_t* offsets;   /* CSR offsets [n_rows + 1]                                  */
    const int32_t* items;     /* corpus positions, ascending within a CSR row;             */
                              /* duplicates allowed; entries >= nx are ignored              */
    int64_t        n_rows;
    const int64_t* rows;      /* optional [nq]: query q uses CSR row rows[q] (NULL: row q); */
                              /* a row outside [0, n_rows) = no exclusions                  */
} RtExclusionLists;

#define RT_ONLINE_MAX_EXCL_SOURCES 2
int rt_flatip_topk_online_lists(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                                int k, const RtExclusionLists* lists, int n_lists, int64_t id_offset,
                                float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------
 * IVF-Flat (faiss.index_factory(d, "IVF1024,Flat") with index.nprobe = 20,
 * the reference's default index: src/serving/retrieval.py:60-62, 101-133;
 * searched at :141-197).
 *
 * rt_ivf_topk: top-k over the union of the probed lists (the scan that
 *   faiss.IndexIVFFlat.search runs after its coarse quantiser, :171).
 *   queries [nq, d] and rows [nx, d], both `dtype`, rows 16-byte aligned; d and
 *   dtype limits of rt_flatip_topk_online (f32: d % 4 == 0, f16/bf16: d % 8 ==
 *   0, d <= 256); 1 <= k <= RT_IVF_MAX_K; 1 <= nprobe <= RT_IVF_MAX_NPROBE;
 *   nq <= 65,535 per call; nx < 2^31 - 1.
 *   rows are stored list-contiguous: list l is the stored rows
 *   [list_offsets[l], list_offsets[l + 1]) (int64 [nlist + 1], device);
 *   row_pos[i] (int32 [nx], device) is the ORIGINAL corpus position of stored
 *   row i. probes (int64 [nq, nprobe], device): list ids, exactly what
 *   rt_flatip_topk / rt_flatip_topk_online write as out_ids over the
 *   centroids; an entry of -1 or outside [0, nlist) is skipped; a list named
 *   twice in a probe row may repeat its rows in the result, nothing worse.
 *   max_list_rows (host): an upper bound of the longest list; with nq and
 *   nprobe it fixes the grid, so the call makes no host read, is
 *   stream-ordered and can be captured in a graph. A list longer than
 *   max_list_rows is the caller's error: its rows past the bound are not
 *   scanned; nothing outside the list or the corpus is ever read, whatever
 *   the offsets hold, and a row whose row_pos is outside [0, nx) is dropped.
 *   exclude_bits: optional uint32 [nq, exclude_words], indexed by ORIGINAL
 *   position (the convention of rt_flatip_topk); exclude_words >=
 *   ceil(nx / 32).
 *   Result rows: the contract of rt_flatip_topk over the union of the probed
 *   lists — the first k in (score desc, original position asc) order,
 *   out_ids = original position, unfilled slots (-FLT_MAX, -1); fp32 scores
 *   are the sequential fmaf chain (bit-identical to the oracle), f16/bf16
 *   scores the same chain over the widened elements. With every list probed
 *   the result is rt_flatip_topk's over the corpus in original order, bit
 *   for bit.
 *   Status, before any device work: RT_ERR_INVALID for a NULL operand
 *   (rows / row_pos may be NULL when nx == 0), k <= 0, nprobe <= 0, nlist <=
 *   0, a negative size, an unknown dtype, misaligned queries / rows /
 *   workspace (8 bytes), exclude_words too small; RT_ERR_UNSUPPORTED for
 *   k > RT_IVF_MAX_K, nprobe > RT_IVF_MAX_NPROBE, nq > 65,535, a refused
 *   d / dtype pair, nx >= 2^31 - 1; RT_ERR_WORKSPACE. nq == 0: RT_OK.
 * rt_ivf_topk_lists: rt_ivf_topk with the bitmap replaced by up to
 *   RT_ONLINE_MAX_EXCL_SOURCES CSR sources that the scan reads itself;
 *   RtExclusionLists means what it means for rt_flatip_topk_online_lists:
 *   query q uses CSR row rows ? rows[q] : q of each source, a CSR row outside
 *   [0, n_rows) excludes nothing, items ascend within a CSR row, duplicates
 *   are allowed, items >= nx are ignored. Items are ORIGINAL corpus positions:
 *   the space of row_pos values, of exclude_bits and of out_ids. A query skips
 *   the union of its CSR rows over all sources. Any list length; a list may
 *   exclude every probed row (then every slot is (-FLT_MAX, -1)). A CSR row
 *   that does not ascend gives unspecified exclusions for that query and
 *   nothing worse: no read falls outside [offsets[r], offsets[r + 1]) of
 *   `items` (offsets[r + 1] < offsets[r] is an empty row). A lane whose row
 *   passed the range and threshold tests looks its position up by bisection —
 *   the order of row_pos plays no part; CSR rows of up to 8,960 entries per
 *   query (all sources together) are searched in LDS, longer ones in global
 *   memory. n_lists == 0: rt_ivf_topk without a bitmap, bit for bit.
 *   Workspace (rt_ivf_topk_workspace_bytes), plan (rt_ivf_topk_plan), result
 *   order and score bits are rt_ivf_topk's; every nq <= 65,535 is served (a
 *   scan block serves one query).
 *   Status, before any device work: RT_ERR_INVALID for n_lists < 0, lists ==
 *   NULL with n_lists > 0, a source with offsets == NULL, n_rows < 0, or items
 *   == NULL with n_rows > 0; RT_ERR_UNSUPPORTED for n_lists >
 *   RT_ONLINE_MAX_EXCL_SOURCES; then every refusal of rt_ivf_topk.
 * rt_ivf_topk_lens, rt_ivf_topk_lists_lens: rt_ivf_topk and rt_ivf_topk_lists
 *   over lists stored with slack (rt_ivf_lists_update below), with two more
 *   operands. list_len (int64 [nlist], device, not NULL): list l is the stored
 *   rows [off[l], off[l] + min(max(list_len[l], 0), off[l + 1] - off[l])),
 *   clamped to [0, nx) as before. n_pos (host): positions are valid in
 *   [0, n_pos) — a row whose row_pos is outside it (the -1 of an empty slot) is
 *   dropped; exclude_words >= ceil(n_pos / 32); exclusion items >= n_pos are
 *   ignored; n_pos < 2^31 - 1. nx is the number of stored rows (the total
 *   capacity) and max_list_rows an upper bound of the largest CAPACITY: the
 *   grid depends on host arguments only, so a captured call stays valid while
 *   lists change in place. The same scan and finish: results, score bits,
 *   workspace, plan and refusals are those of the entry point without _lens
 *   (plus RT_ERR_INVALID for list_len == NULL or n_pos < 0, RT_ERR_UNSUPPORTED
 *   for n_pos >= 2^31 - 1).
 * rt_ivf_topk_plan: host only. out = {chunks per list, rows per chunk, scan
 *   blocks}: a probed list is scanned by `chunks` blocks of `rows per chunk`
 *   rows (a multiple of 256; chunks x rows >= max_list_rows), blocks = nq x
 *   nprobe x chunks, and nprobe x chunks <= 512 (the finish's lists per query).
 *   The smallest chunk that rule allows: at nq = 1 the blocks are all the
 *   parallelism a call has.
 * rt_ivf_topk_workspace_bytes: the partial lists [nq][k][nprobe x chunks] of
 *   8-byte composite keys (256 for a refused shape).
 * rt_ivf_topk_tuning: process-wide floor of the chunk, in 256-row tiles
 *   (0 = the default, 1), for measurements; changes the plan, never a result.
 *
 * rt_segment_mean_f32: the centroid update of one Lloyd step (the mean that
 *   faiss.Clustering.train computes per centroid inside index.train, :131).
 *   rows [n, d] of `dtype` (d / dtype limits as above, 16-byte aligned)
 *   grouped by segment; offsets int64 [n_seg + 1] (device): segment s is the
 *   rows [offsets[s], offsets[s + 1]), clamped to [0, n]. out[s] (fp32
 *   [n_seg, d]) = the mean of the segment's rows, accumulated in fp64 in an
 *   order that depends on the segment's length and d only (no atomics: the
 *   same input gives the same bits), rounded once to fp32; an empty segment
 *   copies prev[s] (fp32 [n_seg, d]); normalize != 0 rescales every non-empty
 *   result to unit L2 norm in fp64 before the rounding (spherical k-means for
 *   the cosine metric; a zero mean stays zero).
 *   Status: RT_ERR_INVALID for a NULL offsets / prev / out (rows may be NULL
 *   when n == 0), negative sizes, d <= 0, an unknown dtype, misaligned rows;
 *   RT_ERR_UNSUPPORTED for a refused d / dtype pair. n_seg == 0: RT_OK.
 * ------------------------------------------------------------------------ */
#define RT_IVF_MAX_K 128
#define RT_IVF_MAX_NPROBE 128
int rt_ivf_topk_tuning(int min_chunk_tiles);
int rt_ivf_topk_plan(int64_t nq, int nprobe, int64_t max_list_rows, int64_t* out);
size_t rt_ivf_topk_workspace_bytes(int64_t nq, int nprobe, int64_t max_list_rows, int k);
int rt_ivf_topk(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                const int64_t* list_offsets, int64_t nlist, const int32_t* row_pos, const int64_t* probes,
                int nprobe, int64_t max_list_rows, int k, const uint32_t* exclude_bits, int64_t exclude_words,
                float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);
int rt_ivf_topk_lists(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                      const int64_t* list_offsets, int64_t nlist, const int32_t* row_pos, const int64_t* probes,
                      int nprobe, int64_t max_list_rows, int k, const RtExclusionLists* lists, int n_lists,
                      float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);
int rt_ivf_topk_lens(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                     const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                     const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                     const uint32_t* exclude_bits, int64_t exclude_words, float* out_scores, int64_t* out_ids,
                     void* workspace, size_t workspace_bytes, void* stream);
int rt_ivf_topk_lists_lens(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                           const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                           const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                           const RtExclusionLists* lists, int n_lists, float* out_scores, int64_t* out_ids,
                           void* workspace, size_t workspace_bytes, void* stream);
int rt_segment_mean_f32(const void* rows, int64_t n, int d, int dtype, const int64_t* offsets, int64_t n_seg,
                        const float* prev, int normalize, float* out, void* stream);

/* ------------------------------------------------------------------------
 * IVF-Flat, list-major batch search: faiss.IndexIVFFlat.search with a batch
 * of users (src/serving/retrieval.py:141-197 at Q in the thousands, and the
 * offline evaluation), where rt_ivf_topk reads a list again for every (query,
 * probe) pair that names it.
 *
 * rt_ivf_topk_batch: the operands, limits and result contract of rt_ivf_topk
 *   (list_len == NULL: lists without slack, n_pos is ignored in favour of nx)
 *   or of rt_ivf_topk_lens (list_len != NULL: the first list_len[l] rows of a
 *   list's capacity are live, positions are valid in [0, n_pos),
 *   max_list_rows bounds the largest capacity); exclude_bits may be NULL. For
 *   every operand set those two accept, out_scores and out_ids are theirs BIT
 *   FOR BIT, for fp32, f16 and bf16: the first k of the union of the probed
 *   lists in (score desc, original position asc) order, (-FLT_MAX, -1) pads;
 *   a probe entry of -1 or outside [0, nlist) is skipped; a list named twice
 *   in a probe row may repeat its rows, nothing worse; rows past
 *   max_list_rows are not scanned; nothing outside a list's window clamped to
 *   [0, nx) is ever read, whatever the offsets hold; a row whose row_pos is
 *   outside the valid range is dropped. Scores are the sequential fmaf chain
 *   over d of the oracle, computed by the fp32 MFMA (one accumulation chain
 *   per score, d ascending; only k-steps inside d are issued); f16 / bf16
 *   elements are widened to fp32 first. No 16-bit MFMA: which path serves a
 *   call never changes a result.
 *   Work: the (query, probe slot) pairs are grouped by list on the device
 *   (integer counting and a prefix scan); a work item is (list, tile of QT
 *   queries that probe it, row chunk) and scans its rows ONCE for the tile.
 *   Six launches, stream-ordered, no host read; the grid
 *   depends on host arguments only (the plan's bound of the work items,
 *   surplus blocks leave), so a captured call may be replayed after probes,
 *   queries or the lists changed in place. CSR exclusion lists are not taken
 *   (rt_ivf_topk_lists remains the small-call path).
 *   Limits: the d / dtype pairs of rt_ivf_topk; 1 <= k <= RT_IVF_MAX_K;
 *   1 <= nprobe <= RT_IVF_MAX_NPROBE; nq x nprobe < 2^31 - 1; nx, n_pos <
 *   2^31 - 1; nlist < 2^31 - 1; the plan's blocks < 2^31 - 1.
 *   Status, before any device work: RT_ERR_INVALID for a NULL operand (rows /
 *   row_pos may be NULL when nx == 0), k <= 0, nprobe <= 0, nlist <= 0, a
 *   negative size, an unknown dtype, misaligned queries / rows (16 bytes) or
 *   workspace (8 bytes), exclude_words < ceil(n_pos / 32); RT_ERR_UNSUPPORTED
 *   for a limit above; RT_ERR_WORKSPACE. nq == 0: RT_OK without a launch.
 * rt_ivf_topk_batch_plan: host only. out = {QT, rows per chunk, chunks per
 *   list, upper bound of the work items, scan blocks launched}. QT = 32; rows
 *   per chunk is a multiple of the scan's 128-row tile: min(8, tiles of
 *   max_list_rows) tiles, more where nprobe x chunks <= 512 (the finish's
 *   lists per query) demands it; chunks x rows per chunk >= max_list_rows;
 *   bound = (floor(P / QT) + min(nlist, P)) x chunks with P = nq x nprobe;
 *   blocks = bound. RT_ERR_INVALID for a non-positive nq, nprobe, nlist or k,
 *   a negative max_list_rows or out == NULL; RT_ERR_UNSUPPORTED for a refused
 *   shape.
 * rt_ivf_topk_batch_workspace_bytes: 8 nq k nprobe chunks (the partial lists
 *   [nq][k][nprobe x chunks] of composite keys) + 4 (3 nlist + 2 + 2 nq
 *   nprobe) (the grouping tables), rounded up to 256; monotone in nq; 256 for
 *   a refused shape.
 * rt_ivf_topk_batch_tuning: process-wide, for measurements only: a bit mask
 *   of the stages a call issues — 1 grouping (the fill and three launches),
 *   2 scan, 4 finish; 0 = the default, all. A stage alone reads what an
 *   earlier whole call left in the same workspace; anything but the default
 *   leaves out_scores / out_ids unspecified. RT_ERR_INVALID outside [0, 7].
 * ------------------------------------------------------------------------ */
int rt_ivf_topk_batch_tuning(int stages);
int rt_ivf_topk_batch_plan(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows, int k, int64_t* out);
size_t rt_ivf_topk_batch_workspace_bytes(int64_t nq, int nprobe, int64_t nlist, int64_t max_list_rows, int k);
int rt_ivf_topk_batch(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                      const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                      const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                      const uint32_t* exclude_bits, int64_t exclude_words,
                      float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Category filters: the request schema's filter_categories
 * (src/api/schemas.py:21-34), tested by the scan itself.
 *
 * Every item carries `tags`, a 64-bit set: bit j = the item belongs to
 * category j of a vocabulary of at most 64 names; 0 = untagged. A query
 * carries two 64-bit masks. Item p is ELIGIBLE for query q iff
 *     (any_of[q] == 0 || (tags[p] & any_of[q]) != 0) && (tags[p] & none_of[q]) == 0
 * so an untagged item passes no non-zero any_of and fails no none_of, and
 * any_of == none_of == 0 filters nothing. A filtered search is the existing
 * search over the eligible items: the same score bits, the same (score desc,
 * original position asc) order and (-FLT_MAX, -1) pads, exact over the rows
 * scanned (k results whenever k eligible rows exist among them; for the IVF
 * entry point the rows scanned are the probed lists). Exclusion lists compose
 * by union of what is skipped.
 *   RtTagFilter: device pointers, 8-byte aligned. item_tags is indexed by the
 *   position the result ids name before id_offset: the local row for the Flat
 *   scan, the ORIGINAL position (the space of row_pos values) for the IVF
 *   scan, [nx] resp. [n_pos] words. any_of / none_of are [nq] or NULL (all 0).
 * rt_flatip_topk_online_tags: rt_flatip_topk_online_lists plus `filter`.
 *   filter == NULL: rt_flatip_topk_online_lists, bit for bit. Otherwise one
 *   instantiation of the same scan serves the filter and 0..2 list sources: a
 *   lane's 8 bytes of tags are one coalesced load per 256-row tile, issued a
 *   tile ahead of the selection that reads them; the masks sit in LDS; an
 *   ineligible row is never appended. Workspace, plan, limits and result rows
 *   are rt_flatip_topk_online's.
 *   Status, before any device work: RT_ERR_INVALID for filter != NULL with
 *   item_tags == NULL while nx > 0 or with a pointer that is not 8-byte
 *   aligned; then every refusal of rt_flatip_topk_online_lists.
 * rt_ivf_topk_tags: rt_ivf_topk_lists_lens plus `filter`; list_len may be NULL
 *   (lists without slack: n_pos is ignored in favour of nx, as
 *   rt_ivf_topk_batch does). filter == NULL: rt_ivf_topk_lists (list_len ==
 *   NULL) or rt_ivf_topk_lists_lens, bit for bit. Otherwise a lane gathers
 *   item_tags[row_pos[row]] under the scores, and only for a position inside
 *   [0, n_pos): the -1 of an empty slot reads nothing. The lists' layout and
 *   rt_ivf_lists_update know nothing of the tags.
 *   Status, before any device work: RT_ERR_INVALID for filter != NULL with
 *   item_tags == NULL while positions exist (n_pos resp. nx > 0) or with a
 *   pointer that is not 8-byte aligned; then every refusal of
 *   rt_ivf_topk_lists(_lens).
 * rt_tag_filter_bitmap: the filter as an exclusion bitmap uint32 [nq, words]
 *   for the entry points that take exclude_bits (rt_flatip_topk,
 *   rt_ivf_topk_batch, calls above the online limits): bit p of row q is set
 *   for every INELIGIBLE p < n_items. accumulate != 0 ORs into what is there
 *   (an exclude_ids bitmap composes); otherwise every word of the row is
 *   overwritten, bits >= n_items zero. Coalesced tag loads, a wave's ballot is two
 *   words, one word stored per thread; no [nq, n_items] intermediate. any_of / none_of may be NULL (all 0).
 *   Status: RT_ERR_INVALID for a negative size, item_tags == NULL while
 *   n_items > 0, bits == NULL while words exist, a pointer that is not 8-byte
 *   (bits: 4-byte) aligned, words < ceil(n_items / 32). nq == 0: RT_OK.
 * ------------------------------------------------------------------------ */
typedef struct {
    const uint64_t* item_tags;  /* [n_pos], by ORIGINAL position (Flat: local row), device */
    const uint64_t* any_of;     /* [nq] or NULL (= all 0), device */
    const uint64_t* none_of;    /* [nq] or NULL (= all 0), device */
} RtTagFilter;

int rt_flatip_topk_online_tags(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                               int k, const RtExclusionLists* lists, int n_lists, const RtTagFilter* filter,
                               int64_t id_offset, float* out_scores, int64_t* out_ids, void* workspace,
                               size_t workspace_bytes, void* stream);
int rt_ivf_topk_tags(const void* queries, int64_t nq, const void* rows, int64_t nx, int d, int dtype,
                     const int64_t* list_offsets, int64_t nlist, const int64_t* list_len, int64_t n_pos,
                     const int32_t* row_pos, const int64_t* probes, int nprobe, int64_t max_list_rows, int k,
                     const RtExclusionLists* lists, int n_lists, const RtTagFilter* filter, float* out_scores,
                     int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);
int rt_tag_filter_bitmap(const uint64_t* item_tags, int64_t n_items, const uint64_t* any_of,
                         const uint64_t* none_of, int64_t nq, uint32_t* bits, int64_t words, int accumulate,
                         void* stream);

/* ------------------------------------------------------------------------
 * MMR re-ranking of retrieved candidates: the ranking stage of the request
 * path (src/serving/service.py:204-228 retrieves num_recommendations * 10
 * candidates and hands them to a second stage that keeps num_recommendations;
 * with no ranker installed it truncates). Maximal Marginal Relevance
 * (Carbonell & Goldstein, SIGIR 1998) needs nothing but the candidates' own
 * stored rows, which are resident.
 *
 * rt_mmr_rerank: per query, a greedy choice of k of its n_cand candidates.
 *   cand_scores / cand_ids [nq, n_cand], contiguous: what rt_flatip_topk,
 *   rt_flatip_topk_online* and rt_ivf_topk* write — scores are the relevance,
 *   ids ORIGINAL corpus positions, pads (-FLT_MAX, -1). rows [n_rows, d] of
 *   `dtype`, 16-byte aligned, d / dtype limits of rt_flatip_topk_online (f32:
 *   d % 4 == 0, f16/bf16: d % 8 == 0, d <= 256). pos_slot: optional int32
 *   [n_pos] (device): the stored row of position p, -1 = none (the array
 *   rt_ivf_lists_update keeps); NULL = the identity (a Flat corpus).
 *   A candidate is ABSENT, wherever it stands in its row, if its id is < 0 or
 *   >= n_pos or its slot is < 0 or >= n_rows; an absent candidate is never
 *   read and never chosen.
 *   lambda: fp32 [nq] on the DEVICE, one value per query, clamped to [0, 1] by
 *   the kernel — data, not a launch argument: one captured graph serves every
 *   lambda.
 *   sim(i, j): normalize == 0: the inner product of the two stored rows,
 *   widened to fp32 (the cosine metric, whose rows are stored unit-norm);
 *   normalize != 0: that inner product times 1/sqrt(|i|^2) times 1/sqrt(|j|^2);
 *   a zero row has similarity 0 to everything (the inner_product metric).
 *   Selection, t = 0 .. k - 1, over the present candidates not yet chosen:
 *   obj(i) = lambda * score_i - (1 - lambda) * m_i, m_i = the maximum of
 *   sim(i, j) over the chosen j (0 while nothing is chosen); the largest obj
 *   is chosen, ties go to the LOWEST CANDIDATE INDEX (the input order).
 *   Duplicate positions among the candidates are legal: each is a candidate
 *   of its own.
 *   out_scores / out_ids [nq, k]: the chosen candidates' ORIGINAL scores and
 *   positions in selection order (the list is no longer score-sorted);
 *   (-FLT_MAX, -1) fills the slots past the number of present candidates.
 *   The outputs must not overlap the inputs.
 *   Determinism: a query's result depends only on its candidate row, the
 *   stored values of those rows, its lambda and normalize — not on nq, its row
 *   index, the grid, or whether pos_slot was given. A dot product is four
 *   sequential fmaf chains (lane l of a candidate takes the 16-byte chunks
 *   l, l + 4, ... of the row, elements ascending) folded as (p0 + p1) + (p2 +
 *   p3); the order depends on (d, dtype) only; no floating-point atomics.
 *   One launch (one workgroup per query, rows staged once in LDS in storage
 *   dtype), no workspace, no host read: stream-ordered and capturable.
 *   Status, before any device work: RT_ERR_INVALID for a NULL operand (rows
 *   may be NULL only when n_rows == 0; pos_slot may always be NULL), k <= 0,
 *   n_cand <= 0, d <= 0, a negative size, an unknown dtype, rows not 16-byte
 *   aligned (the other operands: their element size), out_* overlapping
 *   cand_* or each other; RT_ERR_UNSUPPORTED for n_cand > RT_MMR_MAX_CAND,
 *   k > n_cand, a refused d / dtype pair, n_pos >= 2^31 - 1. nq == 0: RT_OK.
 * ------------------------------------------------------------------------ */
#define RT_MMR_MAX_CAND 128      /* = RT_ONLINE_MAX_K = RT_IVF_MAX_K */
int rt_mmr_rerank(const float* cand_scores, const int64_t* cand_ids, int64_t nq, int n_cand,
                  const void* rows, int64_t n_rows, int d, int dtype,
                  const int32_t* pos_slot, int64_t n_pos,
                  const float* lambda, int normalize, int k,
                  float* out_scores, int64_t* out_ids, void* stream);

/* ------------------------------------------------------------------------
 * In-place mutation of IVF lists stored with slack: the streaming item_update
 * path (RetrievalEngine.update_index, src/serving/retrieval.py:228-246,
 * 629-641) on the reference's default index.
 *
 * State (all device): rows [total_rows, d] of `dtype`, 16-byte aligned;
 *   list_offsets int64 [nlist + 1]: list l OWNS the stored rows
 *   [list_offsets[l], list_offsets[l + 1]) — its capacity; list_len int64
 *   [nlist]: its live rows are the first list_len[l] of them; row_pos int32
 *   [total_rows]: the position of a stored row, -1 in every slot at or past
 *   list_len[l]; pos_slot int32 [total_rows]: the stored row of a position
 *   (-1: none); assign int64 [total_rows]: the list of a position (-1: none).
 *   Positions live in [0, total_rows).
 * rt_ivf_lists_update: one stream-ordered call (a memset of `status` and
 *   three launches; no host read, capturable) for m operations. positions
 *   int64 [m], UNIQUE (the caller's contract, as for rt_scatter_rows);
 *   new_list int64 [m]: what rt_flatip_topk with k = 1 writes over the
 *   centroids, or -1 = the position's row leaves; new_rows [m, d] of `dtype`,
 *   16-byte aligned (read for new_list >= 0 only). Per operation: a position
 *   whose current list equals new_list has its row overwritten where it lies;
 *   otherwise it leaves its current list (if it has a row) and joins new_list
 *   (if >= 0). After the call every touched list holds its old live rows minus
 *   the leavers plus the joiners in its first list_len[l] slots, row_pos = -1
 *   behind them, and pos_slot / row_pos / assign agree.
 *   Placement rule (the same state and batch give the same bytes): per list,
 *   holes = the slots of its leavers in ascending slot order, joiners in
 *   ascending operation order; joiner j takes hole j; surplus joiners append
 *   at the old length; surplus holes below the new length take the surviving
 *   rows at or past the new length, both in ascending slot order. One
 *   workgroup owns a list; rows move as 16-byte vectors.
 *   status int32 [2] (device, written by the call): all or nothing —
 *   status[0] = the number of lists whose new length would exceed their
 *   capacity, status[1] = the number of refused operations (a position outside
 *   [0, total_rows), a new_list outside [-1, nlist), a position whose pos_slot /
 *   assign / row_pos entries do not name each other). If either is non-zero
 *   NOTHING else is written. The caller reads the pair afterwards (8 bytes).
 *   Positions that are not unique: unspecified list contents, nothing is
 *   written outside the state buffers.
 *   Status, before any device work: RT_ERR_INVALID for negative sizes, nlist <=
 *   0, d <= 0, an unknown dtype, misaligned rows / new_rows / workspace (4
 *   bytes), then (m > 0) any NULL operand; RT_ERR_UNSUPPORTED for a refused
 *   d / dtype pair (those of rt_ivf_topk), total_rows, m or nlist >= 2^31 - 1;
 *   RT_ERR_WORKSPACE. m == 0: RT_OK without a launch.
 * rt_ivf_lists_update_workspace_bytes: 4 x (5 m + 3 nlist) bytes rounded up to
 *   256 (negative arguments count as 0); monotone in both.
 * ------------------------------------------------------------------------ */
size_t rt_ivf_lists_update_workspace_bytes(int64_t nlist, int64_t m);
int rt_ivf_lists_update(void* rows, int64_t total_rows, int d, int dtype, const int64_t* list_offsets,
                        int64_t nlist, int64_t* list_len, int32_t* row_pos, int32_t* pos_slot, int64_t* assign,
                        const int64_t* positions, const int64_t* new_list, const void* new_rows, int64_t m,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Corpus-sharded search with ONE corpus-wide threshold per query (several
 * GPUs, each holding a row shard of the corpus that faiss.IndexFlatIP.search
 * would scan whole, src/serving/retrieval.py:141-197): every rank samples its
 * shard, the ranks' samples give each query a threshold that is, w.h.p., at
 * most its k-th score over the WHOLE corpus, and each rank keeps only its
 * rows at or above it — so a query's candidates per shard shrink with the
 * number of shards instead of staying ~k per shard.
 *   rt_flatip_topk_shard_sample: top32 [nq][32] = per query the union of each
 *     lane half's 16 largest group maxima (max of 16 rows) over every
 *     stride-th 128-row stage of the shard, merged and sorted descending
 *     (-inf padded): a subset of the 32 largest sampled group maxima, so a
 *     threshold taken from it is <= the one the exact 32 would give (safe:
 *     only more candidates). stage_counts = {sampled stages, stages} of this
 *     shard.
 *   rt_flatip_topk_shard_plan: host only (no device work): RT_OK and the
 *     stage_counts rt_flatip_topk_shard_sample would report for a shard of
 *     nx rows, or RT_ERR_UNSUPPORTED when the shape has no v4 plan — so every
 *     rank can derive every shard's counts (and whether the global-threshold
 *     path applies on all of them) from the shard sizes alone, without a
 *     collective or a device->host read.
 *   rt_topk_sample_rank: the failure-safe rank (P(threshold > k-th) < 1e-6)
 *     for the sampled fraction sum(sampled) / sum(stages) over all shards
 *     (0 = none fits: search from -inf).
 *   rt_topk_sample_threshold: thr[q] = the rank-th largest of the union of
 *     n_lists (<= 64) such lists (layout [n_lists][nq][32], e.g. all-gathered
 *     over ranks); -FLT_MAX when the union has fewer finite entries.
 *   rt_flatip_topk_shard_search: this shard's rows with score >= thr[q], the
 *     best k of them per query in (score desc, id asc) order, padded with
 *     (-FLT_MAX, -1) when fewer pass. The caller merges the shards' lists;
 *     a query whose merged list holds < min(k, corpus rows) entries had a
 *     threshold above its k-th and is searched again from -inf.
 * f16/bf16 with d % 8 == 0, d <= 128, k <= 128, one query chunk (the v4
 * kernel plan of rt_flatip_topk); RT_ERR_UNSUPPORTED otherwise. The
 * workspace (rt_flatip_topk_shard_workspace_bytes, 0 = unsupported) serves
 * both the sample and the search of the same shape. */
size_t rt_flatip_topk_shard_workspace_bytes(int64_t nq, int64_t nx, int d, int dtype, int k);
int rt_flatip_topk_shard_plan(int64_t nq, int64_t nx, int d, int dtype, int k, int stride, int64_t* stage_counts);
int rt_flatip_topk_shard_sample(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                                int k, int stride, float* top32, int64_t* stage_counts, void* workspace,
                                size_t workspace_bytes, void* stream);
int rt_topk_sample_rank(int k, int64_t sampled_stages, int64_t stages, int* rank);
int rt_topk_sample_threshold(const float* lists, int n_lists, int64_t nq, int rank, float* thr, void* stream);
int rt_flatip_topk_shard_search(const void* queries, int64_t nq, const void* items, int64_t nx, int d, int dtype,
                                int k, const float* thr, int64_t id_offset, float* out_scores, int64_t* out_ids,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Planner override of rt_flatip_topk (tests and tuning; process-wide, not
 * thread-safe, results unchanged by any setting). v4_mode: 0 automatic, 1 never
 * the sampled-threshold kernel pair, 2 it wherever legal (16-bit, d <= 128,
 * k <= 128); + 4: per-split thresholds instead of one corpus-wide threshold
 * per query when the items are split; + 8: fp32 corpora of <= 4096 rows keep
 * the fused register-list scan instead of the score-slab GEMM + per-query
 * select pair (the default for them); + 16: a corpus-wide threshold is
 * sampled by every block over the whole corpus (the round-4 form) instead of
 * by one sample-only launch over every split and a per-query threshold pass.
 * v4_stride: sample every stride-th 128-row stage (0 = planner).
 * v4_rank: threshold = rank-th largest sampled group maximum (-1 = planner,
 * 0 = no sample: a running threshold from -inf). Set before sizing the
 * workspace. */
int rt_flatip_topk_tuning(int v4_mode, int v4_stride, int v4_rank);

/* IndexFlatL2 mode (FaissIndex with metric != "cosine", src/serving/retrieval.py:
 * 96-100). rt_l2_augment_f32 writes rows [x, a, 0...] of ld_out >= d + 1 floats:
 * a = 1 for queries (role 0), a = -0.5*||x||^2 for items (role 1; ||x||^2 a
 * sequential fmaf chain); then rt_flatip_topk on the augmented rows (d' =
 * ld_out) ranks items by q.x - ||x||^2/2, i.e. by ascending ||q - x||^2.
 * rt_l2_finish_f32 takes k_sel >= k such candidates per query (sel_ids
 * [nq, k_sel], item index + id_offset into x_aug, -1 = none) and writes the k
 * nearest by Faiss's reported distance (||q||^2 + ||x||^2 - 2 q.x over the first
 * d columns, sequential fmaf norms and dot, clamped at 0), sorted by (distance
 * asc, id asc), into scores/ids [nq, k]; unfilled slots (FLT_MAX, -1). The
 * selection score and the reported distance round differently: exact (equal to
 * Faiss) unless more than k_sel - k items lie within rounding of the k-th
 * distance. With sel_scores ([nq, k_sel], the selection scores rt_flatip_topk
 * returned with sel_ids) and unverified (int32 [nq]) both given, the finish
 * certifies each query: unverified[q] = 0 when no unselected item can reach
 * the k-th distance within a rounding bound, 1 otherwise (the caller then
 * re-selects that query with a larger k_sel). k_sel <= 512; sel_ids may alias
 * ids only when k_sel == k. */
int rt_l2_augment_f32(const float* x, int64_t n, int d, float* out, int ld_out, int role, void* stream);
int rt_l2_finish_f32(const float* q_aug, int ld_q, const float* x_aug, int ld_x, int d, int64_t nq, int k_sel,
                     const int64_t* sel_ids, const float* sel_scores, int k, float* scores, int64_t* ids,
                     int32_t* unverified, int64_t id_offset, void* stream);

/* Merge n_lists candidate lists per query, layout [n_lists][nq][k_in] (as an
 * all_gather_into_tensor over ranks produces), into the (score desc, id asc)
 * top k_out. id -1 entries are ignored; ids must be < 2^32 - 1; k_out <= 512. */
int rt_topk_merge(const float* scores, const int64_t* ids, int64_t nq, int n_lists, int k_in,
                  int k_out, float* out_scores, int64_t* out_ids, void* stream);

/* On-device negative sampling (sample_negative_items, src/data/movielens.py:
 * 488-512, called per sample by src/training/datasets/movielens.py:104-108).
 * Per row r: num_neg distinct items uniform over [0, num_items) minus the
 * positives of user users[r] (CSR: pos_items[pos_offsets[u] .. pos_offsets[u+1])
 * sorted ascending, unique); if that pool has <= num_neg items, the pool in
 * increasing order followed by -1. Counter-based RNG: the draw is a pure
 * function of (seed + *seed_offset, row, slot, round). num_neg <= 64,
 * num_items < 2^31. out [n, num_neg] int64. */
int rt_sample_negatives(const int64_t* pos_offsets, const int32_t* pos_items, int64_t n_users,
                        const int64_t* users, int64_t n, int64_t num_items, int num_neg, uint64_t seed,
                        const uint64_t* seed_offset, int64_t* out, void* stream);

/* Device batch cursor of a graph-captured epoch (rtrec_amd FeederGraph; the
 * DataLoader batches of src/training/datasets/movielens.py:86-134 over a
 * shuffled interaction list). state = int64 [2] device {batch cursor b,
 * sampler salt}. rt_feeder_batch: row t < batch of batch b is interaction
 * order[b·batch + t]: users[t] = inter_u[row], pos[t] = inter_m[row]
 * (order holds >= (b+1)·batch entries). rt_feeder_commit (one thread, after
 * the step): losses[b] = loss[0], then b += 1 and salt += 1 (the salt is the
 * seed_offset of the batch's rt_sample_negatives). */
int rt_feeder_batch(const int64_t* order, const int64_t* inter_u, const int64_t* inter_m, const int64_t* state,
                    int64_t batch, int64_t* users, int64_t* pos, void* stream);
int rt_feeder_commit(const double* loss, double* losses, int64_t n_losses, int64_t* state, void* stream);

/* ------------------------------------------------------------------------
 * Tower MLP (src/models/two_tower.py:56-72,98-134,196-212,238-281):
 * hidden block l = Linear → act → BatchNorm1d → Dropout, final Linear, then
 * F.normalize(p=2, eps=1e-12).
 *
 * rt_linear_fwd_f32 computes one Linear with fused prologue/epilogue:
 *   A row r  = src[ids ? ids[r] : r]                  (ids: fused row gather)
 *   prev_mode 0: a = A (raw input)
 *             1: a = drop(bn(act_prev(A))), BN in train mode: batch mean/biased var
 *                from prev_stats (fp64 [2k]: Σ act_prev(z), Σ act_prev(z)^2 over m
 *                rows), eps; block 0 writes save_mean/save_invstd [k] and updates
 *                running_mean/var (momentum, unbiased var) — BatchNorm1d.train()
 *             2: same with running stats (eval); block 0 writes save_mean/invstd
 *             3: a = drop(act_prev(A))   (no BN: ItemTower.content_projection)
 *   drop: keep with prob 1-p, scale 1/(1-p), mask = hash(drop_seed, r, col)
 *   z = a · Wᵀ + bias   (W [n, k] row-major, n <= 512)  → z_out [m, n]
 *   stats_out (caller-zeroed) += (Σ_r act(z), Σ_r act(z)^2)
 *   l2_out: F.normalize(z, p=2, eps=1e-12) rows, norms_out[r] = ||z[r]||
 *
 * BatchNorm column sums (stats_out / prev_stats / g_stats / g_prev_stats) are
 * fp64 [RT_STAT_SLOTS][2][width]: row block b adds its partial sums into slot
 * b % RT_STAT_SLOTS (bounds same-address atomic contention), consumers sum the
 * slots in slot order. Caller zeroes them before the producing launch.
 * ------------------------------------------------------------------------ */
#ifndef RT_STAT_SLOTS
#define RT_STAT_SLOTS 8
#endif
#if RT_STAT_SLOTS > 15
#error "RT_STAT_SLOTS > 15: the host arenas (rtrec_amd/models/fused.py STAT_SLOTS) hold 16 slot rows, one of them for ticket counters"
#endif

typedef struct {
    const float* src;        /* [src_rows, ld_src] input rows (features or prev z) */
    int64_t src_rows;        /* rows in src (bounds for gather)                       */
    int ld_src;              /* leading dim of src (>= k)                              */
    const int64_t* ids;      /* optional gather ids [m] (NULL = identity)              */
    int64_t m;               /* output rows                                            */
    int k;                   /* input features                                         */
    int n;                   /* output features                                        */
    const float* w;          /* [n, k]                                                 */
    const float* bias;       /* [n] or NULL                                            */
    int prev_mode;           /* 0 raw, 1 BN train, 2 BN eval, 3 act+dropout only        */
    int prev_act;            /* rt_act of the previous block                           */
    const double* prev_stats;/* [RT_STAT_SLOTS][2k] fp64 sums (mode 1)                 */
    const float* bn_gamma;   /* [k]                                                    */
    const float* bn_beta;    /* [k]                                                    */
    float* running_mean;     /* [k] read (mode 2) / updated (mode 1, may be NULL)      */
    float* running_var;      /* [k]                                                    */
    float* save_mean;        /* [k] written by block 0 (modes 1,2; may be NULL)        */
    float* save_invstd;      /* [k]                                                    */
    float bn_eps;
    float bn_momentum;
    float drop_p;            /* dropout prob of the previous block (0 = off)           */
    uint64_t drop_seed;      /* mask seed = drop_seed + (*seed_offset if non-NULL)      */
    const uint64_t* seed_offset; /* device counter (hipGraph replay draws new masks)   */
    float* z_out;            /* [m, n] pre-activation, or NULL                         */
    int act;                 /* activation of THIS block (for stats_out)               */
    double* stats_out;       /* [RT_STAT_SLOTS][2n] accumulated (NULL = skip)          */
    float* l2_out;           /* [m, n] normalized rows (final layer) or NULL          */
    float* norms_out;        /* [m] row norms (with l2_out)                            */
    int64_t* num_batches_tracked; /* prev BN counter, +1 by block 0 in mode 1 (may be NULL) */
    int64_t seg_split;       /* 0, or a multiple of 32 in (0, m): rows [0, seg_split) and
                                [seg_split, m) are two SEPARATE BatchNorm batches (two tower
                                calls — e.g. positives then negatives through the item
                                tower — in one launch). Every per-column BN buffer above and
                                below (prev_stats, save_mean/invstd, stats_out) is then
                                [2][...] (segment-major), running stats are updated segment 0
                                then segment 1, num_batches_tracked += 2. */
    double* zero_buf;        /* optional fp64 [zero_words] set to 0 by the launch before any
                                other work (a step's first launch clears the next
                                accumulators: loss triple, per-tensor grad norms) */
    int64_t zero_words;
    float* wt_out;           /* optional [k, n]: the launch also writes Wᵀ (row kk = column kk
                                of w), which the backward's dz launch reads as rt_linear_bwd_args.wt
                                (NULL = skip) */
    float* a_out;            /* optional [m, k] (k % 4 == 0, 16-B aligned): the launch also writes
                                the transformed input rows it stages (after the previous block's
                                act / BN / dropout prologue and the gather), which the backward's
                                dW launch reads as rt_linear_bwd_args.a_in (NULL = skip) */
    /* BatchNorm finalised by its producer (optional; with stats_out, a training BN after this
     * Linear): the launch's last block per argument set — found by a ticket counter at word
     * nseg·RT_STAT_SLOTS·2n of stats_out (past the slots; caller-zeroed with them) — turns the
     * column sums into the batch mean / invstd and the running-stat updates ONCE, instead of
     * every block of the consuming launch re-deriving them from the fp64 slots. The consuming
     * launch then passes prev_final = 1 and reads them from its save_mean / save_invstd. */
    float* fin_save_mean;    /* [nseg][n] batch means (the consumer's save_mean); NULL = no finalisation */
    float* fin_save_invstd;  /* [nseg][n] 1/sqrt(biased var + eps) */
    float* fin_running_mean; /* [n] momentum update, segment 0 then segment 1 (NULL = skip) */
    float* fin_running_var;  /* [n] with the unbiased batch variance */
    int64_t* fin_num_batches_tracked; /* += nseg (NULL = skip) */
    float fin_eps;
    float fin_momentum;
    int prev_final;          /* prev_mode 1 only: 1 = the producing launch finalised the batch
                                statistics (save_mean / save_invstd hold them; prev_stats, the
                                running stats and num_batches_tracked are not touched here) */
    /* Split-weight planes (DESIGN.md §5 note i): the three bf16 pieces (hi, mid, lo; split3) of a
     * weight, computed ONCE per step by a side task of an earlier launch instead of in registers
     * by every block that uses it. The pieces are the same bits split3 gives, so results are
     * bit-identical to the in-register split. */
    const uint16_t* w_planes;     /* optional [3][n][k] pieces of THIS launch's w (k % 8 == 0, n <= 128,
                                     16-B aligned): the MFMA k-loop reads them (NULL = split w) */
    uint16_t* wt_planes_out;      /* optional [3][k][n]: side task, the pieces of Wᵀ, read by the
                                     backward's dz launch as rt_linear_bwd_args.wt_planes */
    const float* next_w;          /* optional side task: the pieces of another weight [next_n][next_k]
                                     (the next layer's w, for its launch's w_planes; next_k % 8 == 0) */
    uint16_t* next_w_planes;      /* [3][next_n][next_k] */
    int next_n;
    int next_k;
    /* Fragment-ordered weight images: the fp32 values of a weight in the order the
     * lanes of the MFMA k-loops read them, so a wave's W load covers whole 128-byte lines. Written
     * once per step by a side task, read by every row block; values and MFMA order are those of
     * the loads from w / wt, so results are bit-identical. Sizes: rt_linear_w_frag_bytes. */
    const float* w_frag;          /* optional float4 [T][S][4][64] image of THIS launch's w (k % 8 == 0,
                                     n <= 256, 16-B aligned; T = ceil(n/32), S = ceil(k/32)): entry
                                     (t, s, j, l) with c = l & 31, h = l >> 5 holds
                                     w[32t + c][32s + 16(j>>1) + 8h + 4(j&1) + 0..3], zeros past n / k.
                                     NULL = the loads from w. Used when every argument set of the
                                     launch brings one */
    float* next_w_frag;           /* optional side task: that image of next_w [next_n][next_k]
                                     (next_k % 8 == 0, 16-B aligned) */
    float* wt_frag_out;           /* optional side task (n % 8 == 0, 16-B aligned): the dz image of Wᵀ,
                                     float4 [KT][NS][2][64], KT = ceil(k/32), NS = ceil(n/32)·2: entry
                                     (kt, sb, j, l) holds Wᵀ[32kt + c][16sb + 8h + 4j + 0..3], zeros past
                                     k / n; read by the backward's dz launch as rt_linear_bwd_args.wt_frag */
} rt_linear_fwd_args;

int rt_linear_fwd_f32(const rt_linear_fwd_args* args, void* stream);
/* Bytes of a fragment-ordered image of a Linear W [n][k]: transposed == 0 the forward image
 * (rt_linear_fwd_args.w_frag; 0 when k % 8 != 0 or n > 256), else the dz image
 * (rt_linear_bwd_args.wt_frag; 0 when n % 8 != 0 or k > 256). Rows and columns are padded to
 * whole 32-wide tiles: 32·ceil(n/32) · 32·ceil(k/32) · 4. Host-only, no GPU work. */
size_t rt_linear_w_frag_bytes(int n, int k, int transposed);

/* Backward of one Linear and of the block that produced its output gradient.
 *   grad_mode 0: dz = normalize_bwd(dout; l2_out, norms)            (final layer)
 *             1: dz = act'(z)·γ·invstd·(g − Σg/m − x̂·Σg·x̂/m)    (BN train; g_stats)
 *             2: dz = act'(z)·γ·invstd·g                         (BN eval)
 *             3: dz = act'(z)·g                                   (no BN)
 *      with g = d loss/d(BN output) [m, n], x̂ = (act(z) − save_mean)·save_invstd.
 *   dz_ws [m, n] receives dz; dbias += Σ_r dz; dw += dzᵀ·a  (fp32 atomics into
 *   caller-zeroed buffers, one per output element per M-split of at most 32),
 *   a = the forward input of this Linear recomputed by the same prologue
 *   (src/ids/prev_* exactly as passed to rt_linear_fwd_f32).
 *   modes 1/2: dgamma += Σ g·x̂, dbeta += Σ g (read from g_stats; atomic, so two
 *   chains of one tower may run concurrently on different streams).
 *   da = dz·W [m, k] then: dsrc = da (if non-NULL; input gradient, layer 1) and/or
 *   g_prev = drop_bwd_prev(da) with g_prev_stats += (Σ g_prev, Σ g_prev·x̂_prev)
 *   (x̂_prev from src with prev_mean/prev_invstd; prev_mode 1/2 only).
 *   n <= 256 and k <= 512. */
typedef struct {
    int64_t m; int k; int n;
    const float* w;          /* [n, k] */
    float* dw;               /* [n, k] accumulated */
    float* dbias;            /* [n] accumulated or NULL */
    float* dz_ws;            /* [m, n] workspace */
    int grad_mode;
    const float* dout;       /* mode 0: [m, n] */
    const float* l2_out;     /* mode 0: [m, n] */
    const float* norms;      /* mode 0: [m] */
    const float* g;          /* modes 1-3: [m, n] */
    const float* z;          /* modes 1-3: [m, n] pre-activation of this block */
    int act;                 /* this block's activation */
    const double* g_stats;   /* modes 1,2: [RT_STAT_SLOTS][2n] (Σg, Σg·x̂) */
    const float* save_mean;  /* [n] */
    const float* save_invstd;/* [n] */
    const float* bn_gamma;   /* [n] */
    float* dgamma;           /* [n] accumulated or NULL */
    float* dbeta;            /* [n] */
    /* the input A of this linear, recomputed exactly as the forward prologue */
    const float* src; int64_t src_rows; int ld_src; const int64_t* ids;
    int prev_mode; int prev_act;
    const float* prev_mean; const float* prev_invstd;   /* prev block save_mean/invstd */
    const float* prev_gamma; const float* prev_beta;
    float prev_drop_p; uint64_t prev_drop_seed; const uint64_t* seed_offset;
    /* outputs towards the previous block */
    float* g_prev;           /* [m, k] or NULL */
    double* g_prev_stats;    /* [RT_STAT_SLOTS][2k] accumulated, caller zeroes (NULL = skip) */
    float* dsrc;             /* [m, k] input grad (first layer), or NULL */
    int64_t seg_split;       /* as in rt_linear_fwd_args: g_stats, save_mean/invstd,
                                prev_mean/invstd and g_prev_stats are then [2][...] */
    double* dbias_slots;     /* optional fp64 [RT_STAT_SLOTS + 1][n], caller-zeroed: the dz launch
                                adds each row block's column sums of dz (slot = block % SLOTS)
                                and the dW launch folds the slots into dbias — bounded
                                same-address contention; NULL = the dW launch sums dz itself.
                                With fuse_dz the dW launch adds its splits' sums into the slots
                                and the last block of each n-tile folds them; row RT_STAT_SLOTS
                                then holds that launch's per-tile ticket counters (uint64) */
    const float* wt;         /* optional [k, n] = Wᵀ of THIS step's w (rt_linear_fwd_args.wt_out):
                                dA = dz·W then reads contiguous rows of it (NULL = columns of w) */
    int fuse_dz;             /* 1: a layer with no dA (g_prev and dsrc NULL), grad_mode 1-3, a
                                piecewise-linear act and n % 4 == 0 (16-B aligned g, z) computes
                                dz inside its dW launch: the dz launch of the pair is then a no-op
                                and dz_ws is NOT written; dbias, dgamma, dbeta come from the dW
                                launch (ignored when the layer does not qualify) */
    const float* a_in;       /* optional [m, k] = rt_linear_fwd_args.a_out of this step: the dW
                                launch reads A from it as is instead of recomputing it from src /
                                ids / prev_* (those still serve the dz launch); NULL = recompute */
    float* dw_part;          /* optional [splits][n][k] fp32 (splits: rt_linear_bwd_dw_splits):
                                the dW launch STORES each row split's tile sum here instead of
                                adding it into dw with atomics; a later launch folds it (fold_*) */
    const float* fold_src;   /* optional side task of this args' dz launch (fold_in 0) or dW launch
                                (fold_in 1): fold_dst[e] += sum over s < fold_splits of
                                fold_src[s * fold_words + e], in s order, e < fold_words — the
                                fold of an EARLIER launch's dw_part (fold_words % 4 == 0) */
    float* fold_dst;
    int64_t fold_words;
    int fold_splits;
    int fold_in;
    const uint16_t* wt_planes; /* optional [3][k][n] split pieces of Wᵀ (rt_linear_fwd_args.wt_planes_out
                                  of THIS step; n % 8 == 0, 16-B aligned): dA = dz·W reads them instead
                                  of splitting wt / w in registers (bit-identical) */
    const float* wt_frag;      /* optional dz image of Wᵀ (rt_linear_fwd_args.wt_frag_out of THIS step;
                                  n % 8 == 0, k <= 256, 16-B aligned): dA = dz·W reads its W fragments
                                  from it in whole lines (bit-identical). Used when every argument set
                                  of the launch that has a dA brings one; otherwise wt, else w */
} rt_linear_bwd_args;

int rt_linear_bwd_f32(const rt_linear_bwd_args* args, void* stream);
/* 1 when the dz launch of these (1 or 2) argument sets is a no-op because
 * their dW launch computes dz itself (rt_linear_bwd_args.fuse_dz), else 0 —
 * the caller may then skip the dz call. Host-only, no GPU work. */
int rt_linear_bwd_dz_fused(const rt_linear_bwd_args* args, int n_args);
/* Row splits per argument set that rt_linear_bwd_dw_f32_multi(args, n_args) will
 * use (the planner is joint over the n_args sets): the first dimension of
 * their dw_part buffers. Host-only, no GPU work. */
int rt_linear_bwd_dw_splits(const rt_linear_bwd_args* args, int n_args, int64_t* splits);
/* the two launches of rt_linear_bwd_f32, separately (same arguments, same
 * order on one stream): dz/dgamma/dbeta/dA, then dW/dbias from dz_ws. */
int rt_linear_bwd_dz_f32(const rt_linear_bwd_args* args, void* stream);
int rt_linear_bwd_dw_f32(const rt_linear_bwd_args* args, void* stream);
/* Up to two independent Linears in ONE launch (n_args = 1 or 2; e.g. layer l
 * of the user and of the item tower): the same arguments and results as n_args
 * separate calls, with both layers' work sharing the GPU at once (a replayed
 * hipGraph runs parallel stream branches one after the other, so the two
 * towers' chains only overlap when their launches are merged).
 * Replaces the concurrent UserTower/ItemTower calls of the trainer step
 * (src/training/trainers/two_tower.py:104-137). */
int rt_linear_fwd_f32_multi(const rt_linear_fwd_args* args, int n_args, void* stream);
int rt_linear_bwd_dz_f32_multi(const rt_linear_bwd_args* args, int n_args, void* stream);
int rt_linear_bwd_dw_f32_multi(const rt_linear_bwd_args* args, int n_args, void* stream);
/* The dW (+ dbias, + the fused dz of fuse_dz sets) of up to 6 argument sets —
 * every Linear of a tower pair — in ONE launch, enqueued after the dz launches
 * of all of them (dW of a layer needs only that layer's dz and staged input,
 * and nothing needs dW). Sets are validated as by rt_linear_bwd_dw_f32_multi.
 * fuse_dz is decided PER SET here: clear it on the sets of a pair whose dz
 * launch ran (rt_linear_bwd_dz_fused == 0). A set with dw_part stores its row
 * splits' tile sums ([splits][n][k], splits from rt_linear_bwd_dw_joint_splits)
 * for rt_grad_sqnorm_fold; a set without adds them with fp32 atomics. fold_*
 * with fold_in 1 is refused (no tower launch follows). A set the joint kernel
 * has no instantiation for (a recomputing prologue, a 64x64-tile set with
 * unaligned operands or a gather, a k <= 32 set whose dz is not fused) runs as
 * a launch of its own after the joint one, same results. */
int rt_linear_bwd_dw_f32_joint(const rt_linear_bwd_args* args, int n_args, void* stream);
/* Row splits per argument set that rt_linear_bwd_dw_f32_joint(args, n_args)
 * will use. Host-only, no GPU work. */
int rt_linear_bwd_dw_joint_splits(const rt_linear_bwd_args* args, int n_args, int64_t* splits);

/* ------------------------------------------------------------------------
 * Losses (fp32 scores, fp32 accumulation; bf16/f16 inputs widened on load).
 * rt_twotower_loss_fwd_bwd fuses, for B users u, B positives p, B*n_neg
 * negatives q (row i*n_neg+j belongs to user i):
 *   explicit (contrastive_loss, src/models/two_tower.py:406-451):
 *     pos_i = u_i·p_i/τ + ub + ib ; neg_ij = u_i·q_ij/τ ; CE over [pos_i, neg_i·], label 0
 *   in-batch (in_batch_negative_loss, :453-479): S = U·Pᵀ/τ, CE(S, arange B)
 *   loss = w_explicit·L_explicit + w_in_batch·L_in_batch   (trainer :134)
 * and writes d loss / d{u, p, q} (OVERWRITTEN) and accumulates d loss / d{ub, ib}
 * into d_user_bias / d_item_bias (may be NULL). n_neg = 0: the loss is the
 * in-batch CE alone (weight 1, trainer fallback :136); w_in_batch = 0 skips
 * the in-batch term (contrastive_loss alone).
 * loss_out: fp64 [3] = (loss, L_explicit, L_in_batch), caller zeroes.
 * Workspace: rt_twotower_loss_workspace_bytes(B).
 * ------------------------------------------------------------------------ */
size_t rt_twotower_loss_workspace_bytes(int64_t b, int d);
int rt_twotower_loss_fwd_bwd(const void* u, const void* p, const void* q, int dtype, int64_t b,
                             int d, int n_neg, float inv_tau, const float* user_bias,
                             const float* item_bias, float w_explicit, float w_in_batch,
                             double* loss_out, float* du, float* dp, float* dq, float* d_user_bias,
                             float* d_item_bias, void* workspace, size_t workspace_bytes, void* stream);

/* Forward-only variants (validation, TwoTowerModel.forward(compute_loss=True)). */
int rt_twotower_loss_fwd(const void* u, const void* p, const void* q, int dtype, int64_t b, int d,
                         int n_neg, float inv_tau, const float* user_bias, const float* item_bias,
                         float w_explicit, float w_in_batch, double* loss_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* compute_similarity (src/models/two_tower.py:380-404): s_i = u_i·v_i·inv_tau (+ub+ib). */
/* In-batch CE of a data-parallel shard (config C5): S = U·Pᵀ/τ over b local
 * users x n_items in-batch items (all ranks' items, gathered), label of user i =
 * item label_offset + i; loss_out += (L, 0, L) with L = mean_i CE_i over the
 * local users (average over ranks for the global mean). du [b, D] and dp
 * [n_items, D] are OVERWRITTEN with d L / d U, d L / d P (du == NULL: forward
 * only). Replaces in_batch_negative_loss (src/models/two_tower.py:453-479) for
 * the sharded case; b == n_items, label_offset == 0 is the reference loss. */
size_t rt_inbatch_loss_workspace_bytes(int64_t b, int64_t n_items, int d);
int rt_inbatch_loss_fwd_bwd(const void* u, const void* p, int dtype, int64_t b, int64_t n_items, int d,
                            int64_t label_offset, float inv_tau, double* loss_out, float* du, float* dp,
                            void* workspace, size_t workspace_bytes, void* stream);

int rt_similarity_f32(const float* u, const float* v, int64_t b, int d, float inv_tau,
                      const float* user_bias, const float* item_bias, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Optimiser (src/training/trainers/two_tower.py:60-64,144) on ONE flat fp32
 * parameter slab (all tower tensors + biases contiguous) and its grad slab:
 * rt_grad_sqnorm: sumsq_out[t] += Σ g² over tensor t = [offsets[t], offsets[t+1])
 *   (offsets: device int64 [n_tensors+1]; sumsq_out fp64, caller zeroes); also
 *   increments the device step / dropout-seed counters when non-NULL (one
 *   thread), so a replayed hipGraph advances them without extra launches.
 * rt_clip_adam_step: clip_grad_norm_(max_norm): coef = min(1, max_norm /
 *   (sqrt(Σ_t sumsq[t]) + 1e-6)); then torch.optim.Adam with L2 weight decay and
 *   bias correction on g·coef. The step count and learning rate are read from
 *   device memory when step_dev / lr_dev are non-NULL (hipGraph replay), else
 *   from `step` / `lr`. The grads are CONSUMED: every element is zeroed after
 *   use, and zero_buf[0, zero_words) (fp64, may be NULL) is zeroed too — the
 *   next step's accumulators start at zero without memset launches.
 *   zero_buf must not overlap sumsq (blocks read sumsq while others already zero).
 *   n == 0 returns before any launch: zero_buf is NOT zeroed then.
 *   A NaN in sumsq makes coef NaN (as torch.clamp(max=1) keeps it): all of
 *   params / exp_avg / exp_avg_sq become NaN.
 * rt_grad_sqnorm_fold: rt_grad_sqnorm that first folds row-split partial sums
 *   (rt_linear_bwd_args.dw_part of rt_linear_bwd_dw_f32_joint) into the tensors
 *   the n_folds <= RT_GRAD_FOLD_MAX descriptors name (host array, copied at the
 *   call): element e of such a tensor becomes
 *     g[e] + (((p_0[e] + p_1[e]) + p_2[e]) + … + p_{splits-1}[e]),  p_s = part + s·words,
 *   fp32, in ascending split order; it is written back to grads and that value
 *   is squared into the tensor's sum. Tensors without a descriptor, and the
 *   counters, behave exactly as in rt_grad_sqnorm.
 * ------------------------------------------------------------------------ */
#define RT_GRAD_FOLD_MAX 8
typedef struct {
    const float* part;   /* [splits][words] fp32, 16-B aligned */
    int64_t dst_off;     /* the tensor's first element in grads (== offsets[tensor]; multiple of 4) */
    int64_t words;       /* elements of the tensor (multiple of 4) */
    int splits;          /* >= 1 */
    int tensor;          /* index into offsets / sumsq_out; at most one descriptor per tensor */
} rt_grad_fold;
int rt_grad_sqnorm(const float* grads, const int64_t* offsets, int n_tensors, double* sumsq_out,
                   int32_t* step_counter, int64_t* seed_counter, void* stream);
int rt_grad_sqnorm_fold(float* grads, const int64_t* offsets, int n_tensors, double* sumsq_out,
                        int32_t* step_counter, int64_t* seed_counter, const rt_grad_fold* folds,
                        int n_folds, void* stream);
int rt_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                      int64_t n, const double* sumsq, int n_tensors, float max_norm, float lr,
                      const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                      int step, const int32_t* step_dev, double* zero_buf, int64_t zero_words,
                      void* stream);

/* ------------------------------------------------------------------------
 * Tower inference for one request: UserTower.forward in eval mode
 * (src/models/two_tower.py:98-134) as the serving path calls it,
 * `model.get_user_embeddings(...)` on one feature row
 * (src/serving/service.py:286-293) — every Linear, activation, BatchNorm1d
 * (running statistics) and the final F.normalize in ONE launch of ONE
 * workgroup, for m = 1..RT_TOWER_MAX_ROWS rows. Dropout is off (eval).
 *   per row:   a = src[ids ? ids[r] : r][0 : layers[0].k]
 *   per layer: z = a . W^T + bias;  a = act(z);  with bn_gamma != NULL:
 *              a = (a - mean) / sqrt(var + eps) * gamma + beta
 *   normalize: out[r] = z / max(||z||_2, 1e-12) of the last layer's rows;
 *              norms_out[r] = ||z||_2 (optional, with or without normalize).
 * The reference tower sets act and BatchNorm on every Linear but the last
 * (act = RT_ACT_NONE, bn_gamma = NULL there).
 * An id outside [0, src_rows) reads a row of zeros; nothing outside src is
 * read. fp32 fmaf sums throughout. A row's output bits depend neither on m
 * nor on the row's slot in the call.
 * RT_ERR_INVALID: NULL args / src / out / w, m or n_layers out of range, a
 *   width < 1, ld_src < layers[0].k, ids == NULL with src_rows < m, an
 *   incomplete BatchNorm set. RT_ERR_UNSUPPORTED: a width above
 *   RT_TOWER_MAX_WIDTH, or layers[i].k != layers[i-1].n.
 * ------------------------------------------------------------------------ */
#define RT_TOWER_MAX_LAYERS 8
#define RT_TOWER_MAX_ROWS   8
#define RT_TOWER_MAX_WIDTH  512
typedef struct {
    const float* w;        /* [n, k] row-major */
    const float* bias;     /* [n] or NULL */
    int k, n;
    int act;               /* rt_act applied to this Linear's output; RT_ACT_NONE on the last */
    const float* bn_gamma; /* NULL = no BatchNorm after act */
    const float* bn_beta;
    const float* bn_mean;  /* running_mean */
    const float* bn_var;   /* running_var  */
    float bn_eps;
} rt_tower_layer;
typedef struct {
    const float* src; int64_t src_rows; int ld_src;
    const int64_t* ids;    /* optional [m] rows of src (fused gather); NULL = rows 0..m-1 */
    int m;                 /* 1..RT_TOWER_MAX_ROWS */
    int n_layers;          /* 1..RT_TOWER_MAX_LAYERS */
    rt_tower_layer layers[RT_TOWER_MAX_LAYERS];
    int normalize;         /* 1: F.normalize(p=2, eps=1e-12) of the last layer's rows */
    float* out;            /* [m, n_last] */
    float* norms_out;      /* optional [m] */
} rt_tower_infer_args;
int rt_tower_infer_f32(const rt_tower_infer_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Offline evaluation (scripts/evaluate_model.py:162-234, src/evaluation/
 * metrics.py:73-228,248-319).
 *
 * rt_exclusion_bitmap: the train-item mask of generate_recommendations
 *   (evaluate_model.py:224-228: `user_scores[train_item] = -inf` for every
 *   train item < num_items) as the exclude_bits operand of rt_flatip_topk.
 *   Row r uses CSR row u = rows ? rows[r] : r (items sorted ascending, unique;
 *   u outside [0, n_csr_rows) = no exclusions); bits [n_rows, words] uint32,
 *   words >= ceil(n_items/32), every word written.
 *
 * rt_rank_metrics: Evaluator.evaluate per query row r. preds [n_rows,
 *   list_len] int64 ranked item ids (-1 pads a ragged list); ground truth =
 *   CSR row gt_rows ? gt_rows[r] : r (sorted unique items; empty = the row is
 *   skipped, valid[r] = 0, like a user without ground truth); optional
 *   exclusions (CSR, same indirection) are removed from the list before
 *   ranking (metrics.py:279-281). k_values: HOST array of n_k ascending
 *   positive ints, n_k <= RT_METRICS_MAX_K. Predictions must not repeat an item.
 *   per_row fp64 [n_rows][4*n_k + 2] = recall@k[n_k], precision@k[n_k],
 *   ndcg@k[n_k], hit_rate@k[n_k], reciprocal rank, average precision
 *   (the reference's per-user functions, accumulated rank-ascending in fp64).
 *   coverage_bits (optional, caller-zeroed, ceil(num_items/32) words): items
 *   of the first max(k) kept predictions of valid rows (metrics.py:287).
 *
 * rt_rank_metrics_reduce: out fp64 [n_cols + 2] = mean of each per_row column
 *   over valid rows (fixed summation order: deterministic), the number of valid
 *   rows, and coverage = popcount(coverage_bits) / num_items (0 when NULL).
 * ------------------------------------------------------------------------ */
#define RT_METRICS_MAX_K 16

int rt_exclusion_bitmap(const int64_t* offsets, const int32_t* items, int64_t n_csr_rows, const int64_t* rows,
                        int64_t n_rows, int64_t n_items, uint32_t* bits, int64_t words, void* stream);
int rt_rank_metrics(const int64_t* preds, int64_t n_rows, int list_len, const int64_t* gt_offsets,
                    const int32_t* gt_items, const int64_t* gt_rows, int64_t n_gt_rows,
                    const int64_t* ex_offsets, const int32_t* ex_items, const int64_t* ex_rows,
                    int64_t n_ex_rows, const int32_t* k_values, int n_k, int64_t num_items,
                    double* per_row, int32_t* valid, uint32_t* coverage_bits, void* stream);
int rt_rank_metrics_reduce(const double* per_row, const int32_t* valid, int64_t n_rows, int n_cols,
                           const uint32_t* coverage_bits, int64_t num_items, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Beyond-accuracy list metrics (src/evaluation/metrics.py:402-478,
 * scripts/evaluate_model.py:309-338): intra-list diversity and novelty of
 * device-resident rankings, every k in one pass.
 *
 * rt_list_metrics: per row r of preds [n_rows, list_len] int64 (-1 = no
 *   item, the "present" rule of rt_rank_metrics) and per k of k_values (HOST
 *   array of n_k ascending positive ints, n_k <= RT_METRICS_MAX_K), over the
 *   first n = min(k, len(list)) entries of the row's list:
 *   diversity (emb != NULL): mean over pairs i < j of 1 - ê_i·ê_j with
 *     ê = e / (‖e‖ + 1e-8), computed in fp64 on the stored values as
 *     1 - (‖Σ ê_i‖² - Σ ‖ê_i‖²) / (n(n-1)) (no K×K matrix). emb [n_emb, d]
 *     of emb_dtype (rt_dtype) with a row stride of ld_emb >= d elements;
 *     fp32: 1 <= d <= 1024, fp16 / bf16: d % 8 == 0, d <= 1024
 *     (RT_ERR_UNSUPPORTED otherwise). 16-byte loads when d, ld_emb and the
 *     base pointer allow, element loads otherwise. Every id is checked
 *     against n_emb before its row is read; an id >= n_emb is not read, is
 *     counted in oob_count (optional, caller-zeroed) and is left out of the
 *     row's diversity list. div fp64 [n_rows][n_k]; div_valid int32
 *     [n_rows][n_k] = 1 where n >= 2 (else 0 and div = 0).
 *   novelty (info != NULL): info fp64 [n_info] holds each item's
 *     self-information -log2(pop/total + 1e-10); ids >= n_info take
 *     default_info (an item the popularity table does not hold: pop = 1).
 *     nov_sum fp64 [n_rows][n_k] = Σ info over the first n entries, nov_cnt
 *     int32 [n_rows][n_k] = n.
 *   emb and info are each optional (not both NULL); a NULL operand's outputs
 *   are not written. Every argument is validated before any device work;
 *   n_rows == 0 returns RT_OK. No floating-point atomics: two calls on the
 *   same inputs return the same bits.
 *
 * rt_list_metrics_reduce: out fp64 [4][n_k] = the mean of div over the rows
 *   valid at k (0 when none), the number of those rows, Σ nov_sum / Σ nov_cnt
 *   (the reference's flat mean over entries; 0 when none), Σ nov_cnt. A NULL
 *   pair (div, div_valid) or (nov_sum, nov_cnt) gives zeros. Fixed summation
 *   order (deterministic).
 * ------------------------------------------------------------------------ */
int rt_list_metrics(const int64_t* preds, int64_t n_rows, int list_len, const void* emb, int emb_dtype,
                    int64_t n_emb, int d, int64_t ld_emb, const double* info, int64_t n_info, double default_info,
                    const int32_t* k_values, int n_k, double* div, int32_t* div_valid, double* nov_sum,
                    int32_t* nov_cnt, int32_t* oob_count, void* stream);
int rt_list_metrics_reduce(const double* div, const int32_t* div_valid, const double* nov_sum,
                           const int32_t* nov_cnt, int64_t n_rows, int n_k, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RTREC_HIP_H */
