"""Row-ORDERED corpora with exact integer scores, for the Flat-IP top-K tests.

The candidate-buffer scans (csrc/topk_v2.h, topk_v3.h, topk_v4.h) are not
order-independent: passing rows are appended to a fixed-size region per query,
and the region is checked (compacted, the threshold raised) only at certain
points of the loop. How full a region gets depends on WHERE in the row order
the passing rows sit. I.i.d. rows never probe that; these corpora do.

Encoding. A coordinate GROUP is 3 dims. A row whose rank in group g is
r < 2^18 stores the base-64 digits (r >> 12, (r >> 6) & 63, r & 63) on the
group's dims; a query selecting group g with scale c (c = +-1, +-2, +-4) is
(4096 c, 64 c, c) there and 0 elsewhere, so score = c * r. Digits < 64 fit
bf16's 8 significand bits, 4096 * 4 fits f16, every product and every partial
sum is an integer below 2^24: the scores are EXACT in fp32, f16 and bf16
alike, in any summation order. Ranks are distinct inside a group, so there are
no ties and the top-k has a closed form: the rows holding the k largest c * r.
One corpus carries d // 3 orderings at once; each query sees another one.

The second half of the file is the COUNT MODEL of the v4 scan: a mirror of
where the scan stores and where it checks, as it was before the end-of-scan
check was added and as it is now (see count_model).
"""
import functools

import numpy as np

GROUP = 3
MAX_RANK = 1 << 18
SCALES = (1.0, -1.0, 2.0, -2.0, 4.0, -4.0)


def n_groups(d):
    return d // GROUP


# ---- orderings: rank (int64 [nx], distinct) as a function of the row index ----
def ascending(nx, base=0):
    return base + np.arange(nx, dtype=np.int64)


def descending(nx):
    return np.arange(nx, dtype=np.int64)[::-1].copy()


def desc_then_asc(nx, run):
    """Rows [0, nx - run): descending, all below the run; the last `run` rows
    ascend to the top. A running threshold sees every row of the run pass."""
    i = np.arange(nx, dtype=np.int64)
    start = nx - run
    return np.where(i < start, start - 1 - i, i)


def sawtooth(nx, period):
    """Ascending inside every period of `period` rows, distinct overall."""
    i = np.arange(nx, dtype=np.int64)
    nper = -(-nx // period)
    return (i % period) * nper + i // period


def clustered_top(nx, start, block, seed=0):
    """The `block` best rows are rows [start, start + block), ascending; every
    other row holds a low rank (a seeded permutation of 0 .. nx - block - 1)."""
    assert 0 <= start and start + block <= nx
    low = np.random.default_rng(seed).permutation(nx - block).astype(np.int64)
    r = np.empty(nx, np.int64)
    r[:start] = low[:start]
    r[start + block:] = low[start:]
    r[start:start + block] = nx + np.arange(block)
    return r


def bucket_ascending(nx, phase):
    """Ascending ranks in [2^17, 2^18): 1,024 consecutive scores share the top
    16 bits of their fp32 pattern, the key prefix the v2/v3 compaction cuts at.
    Inside such a bucket a compaction keeps everything and every new row still
    passes; `phase` moves the bucket boundaries against the stages."""
    assert (1 << 17) + phase + nx <= MAX_RANK
    return (1 << 17) + phase + np.arange(nx, dtype=np.int64)


# ---- encoding ----
def encode(ranks, d):
    """ranks: int64 [nx, G] with G <= d // 3 -> float32 [nx, d]."""
    ranks = np.asarray(ranks, np.int64)
    nx, g = ranks.shape
    assert g <= n_groups(d) and ranks.min() >= 0 and ranks.max() < MAX_RANK
    x = np.zeros((nx, d), np.float32)
    x[:, 0:GROUP * g:GROUP] = ranks >> 12
    x[:, 1:GROUP * g:GROUP] = (ranks >> 6) & 63
    x[:, 2:GROUP * g:GROUP] = ranks & 63
    return x


def queries(pairs, d):
    """pairs: [(group, scale)] -> float32 [nq, d]."""
    q = np.zeros((len(pairs), d), np.float32)
    for j, (g, c) in enumerate(pairs):
        q[j, GROUP * g:GROUP * g + GROUP] = (4096.0 * c, 64.0 * c, c)
    return q


def closed_form_topk(ranks, pairs, k, exclude=None, id_offset=0):
    """(scores f32 [nq, k], ids int64 [nq, k]) from the ranks alone: the rows
    holding the k largest scale * rank, best first; (-FLT_MAX, -1) padded."""
    nx = ranks.shape[0]
    s_out = np.full((len(pairs), k), -np.finfo(np.float32).max, np.float32)
    i_out = np.full((len(pairs), k), -1, np.int64)
    for j, (g, c) in enumerate(pairs):
        sc = c * ranks[:, g].astype(np.float64)
        rows = np.arange(nx)
        if exclude is not None:
            keep = np.ones(nx, bool)
            keep[np.asarray(exclude[j], np.int64)] = False
            rows = rows[keep]
        order = rows[np.lexsort((rows, -sc[rows]))][:k]
        s_out[j, :order.size] = sc[order]
        i_out[j, :order.size] = order + id_offset
    return s_out, i_out


# ---- the v4 planner's item splits (csrc/topk_api.hip::plan_v4), restated ----
NT = 128          # rows per stage
V4_QT = 512       # queries per v4 block (8 waves x 2 sets of 32)
V4_CAP = 1024     # entries per (split, query) region
V4_ROOM = 896     # kRoom: what a region may hold when a check passes


def v4_splits(nq, nx):
    """(items_per_split, splits) of the v4 plan for one query chunk."""
    q_tiles = -(-min(nq, 65536) // V4_QT)
    splits = 1
    while splits < 16 and q_tiles * splits < 256:
        splits *= 2
    tiles = -(-nx // NT)
    while splits > 1 and tiles // splits < 8:
        splits //= 2
    ips = max(1, -(-tiles // splits)) * NT
    return ips, -(-nx // ips)


# ---- the multi-ordering corpus ----
def multi_corpus(nx, d, nq_plan=512, phase0=0, block=128):
    """One corpus, d // 3 orderings. Returns (x f32 [nx, d], ranks [nx, G],
    names [G]). Groups, in order:
      ascending, [descending at d >= 96], sawtooth(128), [sawtooth(4096) at d >= 96],
      bucket_ascending, clustered tops (d >= 96: first stage / ragged end /
      straddling a v4 split boundary / stage 0 of a split, which every sample
      visits / stages 1-2 of a split, which a stride >= 3 sample skips; d < 96:
      the ragged end and the split boundary only),
      then desc_then_asc runs of 256 + phase0 + step * j rows for every group
      left: step 8 over 32 groups at d = 128 (256 rows, two stages), step 16
      over 16 groups at d = 64 (two nx / phase0 values interleave to step 8)."""
    G = n_groups(d)
    ips, splits = v4_splits(nq_plan, nx)
    mid = ips * max(1, splits // 2)
    cols, names = [], []

    def add(name, r):
        names.append(name)
        cols.append(r)

    add("ascending", ascending(nx))
    if d >= 96:  # (below: a negative scale turns `ascending` into this order)
        add("descending", descending(nx))
    add("sawtooth128", sawtooth(nx, 128))
    if d >= 96:
        add("sawtooth4096", sawtooth(nx, 4096))
    add("bucket_ascending", bucket_ascending(nx, 8 * (nx % 61)))
    tops = [("top_ragged_end", nx - block), ("top_split_boundary", mid - block // 2)]
    if d >= 96:
        tops += [("top_first_stage", 0), ("top_sampled_stage", mid + 3), ("top_skipped_stage", mid + NT + 16)]
    for t, (name, start) in enumerate(tops):
        add(name, clustered_top(nx, min(max(start, 0), nx - block), block, seed=t))
    left = G - len(cols)
    step = 8 if left >= 32 else 16
    for j in range(left):
        run = 256 + phase0 + step * j
        add(f"run{run}", desc_then_asc(nx, run))
    ranks = np.stack(cols, axis=1)
    return encode(ranks, d), ranks, names


def cycle_pairs(n_groups_, nq, scales=SCALES):
    """nq (group, scale) pairs: every group under every scale, cycled."""
    base = [(g, c) for c in scales for g in range(n_groups_)]
    return [base[j % len(base)] for j in range(nq)]


# ---- the count model of the v4 main pass ----
def count_model(rows, first_pass, ring, new, late_set):
    """Peak entry count of ONE candidate region (shared layout: one per split
    and query) over a v4 main pass (csrc/topk_v4.h::main_pass) with an
    EXTERNAL threshold, for a split of `rows` rows of which exactly the rows
    [first_pass, rows) pass. Returns (peak, max count seen by a check,
    compacted).

    What is mirrored, and nothing else:
      * a stage is NT = 128 rows = NSUB = 4 sub-tiles of 32; a ragged last
        stage skips the sub-tiles that start past the end;
      * appends per sub-tile: the passing rows of the sub-tile (both lane
        halves share the region: up to 16 + 16);
      * the lag: the LAST query set of a wave (`late_set`: queries 32..63 of
        every 64) stores sub-tile t while sub-tile t + 1 computes, and its last
        sub-tile in a flush after the loop; the other set stores at once;
      * checks (count > V4_ROOM: compaction). ring = 4 (d = 128): at the end
        of a stage; ring = 3 (d < 128): before the last sub-tile slot of a
        stage. OLD placement (new = False): only in stages that have a
        successor. NEW: in every stage. One more check follows the flush in
        both, after every store: it cannot lower the peak.
      * a compaction keeps between k and V4_ROOM entries: the model takes
        V4_ROOM (an upper bound) and reports compacted = True; with compacted
        = False the counts are exact.
    The kernel's static_assert next to kRoom uses the same derivation."""
    nst = -(-rows // NT)
    cnt = peak = seen = 0
    compacted = False
    prev = None  # the sub-tile the late set holds back

    def passing(t):
        lo, hi = max(32 * t, first_pass), min(32 * t + 32, rows)
        return max(0, hi - lo)

    def store(t):
        nonlocal cnt, peak
        cnt += passing(t)
        peak = max(peak, cnt)

    def check():
        nonlocal cnt, seen, compacted
        seen = max(seen, cnt)
        if cnt > V4_ROOM:
            cnt, compacted = V4_ROOM, True

    for v in range(nst):
        more = v + 1 < nst
        rem = min(NT, rows - v * NT)
        for rt in range(4):
            if ring == 3 and rt == 3 and (more or new):
                check()
            if rt * 32 < rem:
                t = 4 * v + rt
                if late_set:
                    if prev is not None:
                        store(prev)
                    prev = t
                else:
                    store(t)
        if ring == 4 and (more or new):
            check()
    if late_set and prev is not None:
        store(prev)
    return peak, seen, compacted


def mode4_regions(nq, nx, p):
    """The (rows, first_pass) of every split region of a query whose last `p`
    rows of an nx-row ascending corpus pass, under the v4 plan for nq queries."""
    ips, splits = v4_splits(nq, nx)
    out = []
    for s in range(splits):
        b, e = s * ips, min(nx, (s + 1) * ips)
        out.append((e - b, min(max(nx - p - b, 0), e - b)))
    return out


@functools.lru_cache(maxsize=None)
def mode4_peak(nq, nx, p, ring, new, late_set):
    """Worst region of the query: (peak, max count at a check, compacted)."""
    res = [count_model(r, f, ring, new, late_set) for r, f in mode4_regions(nq, nx, p)]
    return max(r[0] for r in res), max(r[1] for r in res), any(r[2] for r in res)


# the deterministic overflow grid (tests/test_gpu_topk_ordered.py, mode 4)
# queries 0 .. 270 pass their last 840 + j rows; queries 271 .. 511 repeat the
# tails rotated, so that 1,025 .. 1,056 — the tails that overflow only the LATE
# set at d = 128 — fall on late-set queries (288 .. 319) and nq = 512 fills the
# block: the last region then borders the entry counts behind the buffer
MODE4_P = tuple(range(840, 1111)) + tuple(840 + (i + 168) % 271 for i in range(241))
MODE4_N_ISSUE = (8192, 8193, 8223, 8224, 8289)
# the same tails on a corpus the planner leaves in ONE split (fewer than 16
# stages): at the sizes above it cuts 8 splits of <= 1,152 rows, no region
# receives more than 1,024 passing rows and 896 + tail is never reached
MODE4_N_ONE_SPLIT = (1152, 1153, 1183, 1184, 1249)
MODE4_N = MODE4_N_ISSUE + MODE4_N_ONE_SPLIT


# ---- the count model of the v3 scan inside one 16-bit key bucket ----
V3_HALF = 256     # entries per lane half (v2::kHalf)
V3_KEEP_OLD = 448  # what a compaction's radix bucket could keep (v2's kCap - 64)
V3_KEEP = 352     # ... and what v3 lets it keep now: 2 * (256 - 64 - 16)


def v3_bucket_model(rows, boundary, k, keep):
    """Peak entries of one lane HALF over a v3 scan (csrc/topk_v3.h) of `rows`
    rows whose scores ascend, rows [0, boundary) inside one 16-bit key bucket
    and rows [boundary, rows) inside the next (bucket_ascending). Mirrored:
      * every row passes (a threshold is a bucket floor, the scores ascend);
        a sub-tile gives each half 16 appends, stored one sub-tile late, the
        last one by the select() after the loop;
      * the check sits at the top of a stage: a half above lim = 2 k + 32
        entries compacts the query. The radix select cuts at the 16-bit prefix
        of the k-th best: the new bucket once it holds k entries, else both.
        Up to `keep` survivors stay, dealt evenly over the halves; more: the
        exact sort leaves k.
    A ragged end only shortens the last stretch; rows is a multiple of 32."""
    lim = min(V3_HALF - 64, 2 * k + 32)
    old = new = 0  # entries of the query (both halves) in the two buckets
    peak = 0
    pending = None
    for t in range(rows // 32):
        if t % 4 == 0 and -(-(old + new) // 2) > lim:  # top of a stage
            if new >= k:
                old = 0
            if old + new > keep:
                old, new = (0, k) if new >= k else (k - new, new)
        if pending is not None:
            if 32 * pending < boundary:
                old += 32
            else:
                new += 32
            peak = max(peak, -(-(old + new) // 2))
        pending = t
    return peak + 16  # the final select()
