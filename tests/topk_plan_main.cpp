// Stand-alone driver of csrc/topk_sample_plan.h for tests/test_topk_plan_cpu.py,
// built there with g++ -fsanitize=address,undefined. argv: k:nx:items_per_split
// triples. Per triple one line "k nx items_per_split stride rank sampled total"
// (the counts at the planned stride, or at stride 1 when no stride fits), after
// asking the memoised planner twice from each of two threads.
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "topk_sample_plan.h"

using namespace rt::topk::splan;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        int k;
        long long nx, ips;
        if (std::sscanf(argv[i], "%d:%lld:%lld", &k, &nx, &ips) != 3) return 2;
        const SamplePlan direct = plan_sample(k, nx, ips);
        SamplePlan got[2][2];
        std::thread t0([&] { for (auto& g : got[0]) g = plan_sample_cached(k, nx, ips); });
        std::thread t1([&] { for (auto& g : got[1]) g = plan_sample_cached(k, nx, ips); });
        t0.join();
        t1.join();
        for (const auto& th : got)
            for (const auto& g : th)
                if (g.stride != direct.stride || g.rank != direct.rank) {
                    std::fprintf(stderr, "memo disagrees at %s\n", argv[i]);
                    return 1;
                }
        const StageCounts c = sampled_stages(nx, ips, direct.stride > 0 ? direct.stride : 1);
        std::printf("%d %lld %lld %d %d %lld %lld\n", k, nx, ips, direct.stride, direct.rank,
                    static_cast<long long>(c.sampled), static_cast<long long>(c.total));
    }
    return 0;
}
