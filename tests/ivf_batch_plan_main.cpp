// Stand-alone driver of csrc/ivf_batch_plan.h for tests/test_ivf_batch_abi_cpu.py:
// built with g++ -fsanitize=address,undefined and run as a child process.
// Each argument is nq:nprobe:nlist:max_list_rows:k; one output line per
// argument: "ok qt rows_per_chunk chunks items_bound blocks workspace_bytes"
// (ok = 0: a refused shape, the rest zeros).
#include <cstdio>
#include <cstdlib>

#include "ivf_batch_plan.h"

int main(int argc, char** argv) {
    namespace ib = rt::topk::ivfb;
    for (int i = 1; i < argc; ++i) {
        long long nq, nprobe, nlist, mlr, k;
        if (std::sscanf(argv[i], "%lld:%lld:%lld:%lld:%lld", &nq, &nprobe, &nlist, &mlr, &k) != 5) {
            std::fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
        ib::Plan p{};
        const bool ok = ib::make_plan(nq, static_cast<int>(nprobe), nlist, mlr, static_cast<int>(k), p);
        if (!ok) {
            std::printf("0 0 0 0 0 0 0\n");
            continue;
        }
        // the plan's own invariants, checked where the sanitizers watch the arithmetic
        if (p.rows_per_chunk % ib::kTileRows != 0 || p.chunks < 1 ||
            static_cast<long long>(p.chunks) * p.rows_per_chunk < mlr || nprobe * p.chunks > ib::kMaxLists ||
            p.blocks != p.items_bound) {
            std::fprintf(stderr, "plan invariant broken for %s\n", argv[i]);
            return 1;
        }
        std::printf("1 %d %lld %d %lld %lld %zu\n", p.qt, static_cast<long long>(p.rows_per_chunk), p.chunks,
                    static_cast<long long>(p.items_bound), static_cast<long long>(p.blocks),
                    ib::workspace_bytes(nq, static_cast<int>(nprobe), nlist, static_cast<int>(k), p));
    }
    return 0;
}
