// Host side of rt_refine_topk under ASan / UBSan: a stand-alone program (its own
// main) that walks the argument checks of the entry point — every call below is
// refused, or has nothing to do, before any device work, so it needs no GPU.
// The source is compiled in, not loaded into another process. `make host-checks`
// in the package directory builds and runs it with its neighbours (mmr_args.cpp
// shows the command by hand; the sources here are csrc/refine.hip csrc/capi.hip).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rtrec_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                      \
    do {                                                                        \
        const int got_ = (call);                                                \
        if (got_ != (want)) {                                                   \
            std::fprintf(stderr, "line %d: got %d, want %d\n", __LINE__, got_, (want)); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

template <typename T>
static T* fake(uintptr_t v) {
    return reinterpret_cast<T*>(v);
}

struct Args {
    // aligned fake pointers, far apart: never dereferenced by a call that is refused
    const float* queries = fake<const float>(1u << 24);
    int64_t nq = 2;
    int d = 64;
    const int64_t* cand_ids = fake<const int64_t>(2u << 24);
    int n_cand = 100;
    const void* store = fake<const void>(3u << 24);
    int64_t n_rows = 1000;
    int kind = RT_REFINE_F32;
    const float* lo = nullptr;
    const float* step = nullptr;
    int k = 10;
    float* out_scores = fake<float>(6u << 24);
    int64_t* out_ids = fake<int64_t>(7u << 24);
};

static int run(const Args& a) {
    return rt_refine_topk(a.queries, a.nq, a.d, a.cand_ids, a.n_cand, a.store, a.n_rows, a.kind, a.lo, a.step, a.k,
                          a.out_scores, a.out_ids, nullptr);
}

int main() {
    const Args ok;
    Args sq8;
    sq8.kind = RT_REFINE_SQ8, sq8.lo = fake<const float>(4u << 24), sq8.step = fake<const float>(5u << 24);
    Args a;
    // ---- RT_ERR_INVALID ----
    a = ok, a.queries = nullptr;
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.cand_ids = nullptr;
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.store = nullptr;                                  // rows exist
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.out_scores = nullptr;
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.out_ids = nullptr;
    EXPECT(run(a), RT_ERR_INVALID);
    a = sq8, a.lo = nullptr;
    EXPECT(run(a), RT_ERR_INVALID);
    a = sq8, a.step = fake<const float>((5u << 24) + 8);        // 16-byte alignment
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.store = fake<const void>((3u << 24) + 8);
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.cand_ids = fake<const int64_t>((2u << 24) + 4);
    EXPECT(run(a), RT_ERR_INVALID);
    for (int v : {0, -1}) {
        a = ok, a.k = v;
        EXPECT(run(a), RT_ERR_INVALID);
        a = ok, a.n_cand = v;
        EXPECT(run(a), RT_ERR_INVALID);
        a = ok, a.d = v;
        EXPECT(run(a), RT_ERR_INVALID);
    }
    for (int kind : {4, -1}) {
        a = ok, a.kind = kind;
        EXPECT(run(a), RT_ERR_INVALID);
    }
    a = ok, a.nq = -1;
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.n_rows = -1;
    EXPECT(run(a), RT_ERR_INVALID);
    a = ok, a.nq = 0, a.k = 0;                                  // refused with no query too
    EXPECT(run(a), RT_ERR_INVALID);

    // ---- RT_ERR_UNSUPPORTED ----
    a = ok, a.n_cand = RT_REFINE_MAX_CAND + 1;
    EXPECT(run(a), RT_ERR_UNSUPPORTED);
    a = ok, a.k = 101;                                          // k > n_cand
    EXPECT(run(a), RT_ERR_UNSUPPORTED);
    for (int64_t nq : {int64_t{65536}, INT64_MAX}) {
        a = ok, a.nq = nq;
        EXPECT(run(a), RT_ERR_UNSUPPORTED);
    }
    for (int d : {260, 66, INT32_MAX}) {
        a = ok, a.d = d;
        EXPECT(run(a), RT_ERR_UNSUPPORTED);
    }
    a = ok, a.d = 68, a.kind = RT_REFINE_BF16;
    EXPECT(run(a), RT_ERR_UNSUPPORTED);
    for (int d : {8, 40, 272}) {
        a = sq8, a.d = d;
        EXPECT(run(a), RT_ERR_UNSUPPORTED);
    }

    // ---- nothing to do ----
    a = ok, a.nq = 0;
    EXPECT(run(a), RT_OK);
    a = ok, a.nq = 0, a.store = nullptr, a.n_rows = 0;          // no rows: store may be NULL
    EXPECT(run(a), RT_OK);
    a = sq8, a.nq = 0, a.d = 256, a.n_cand = 128, a.k = 128, a.n_rows = INT64_MAX;
    EXPECT(run(a), RT_OK);

    std::printf(failures ? "FAILED: %d\n" : "refine_args: OK\n", failures);
    return failures ? 1 : 0;
}
