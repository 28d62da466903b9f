// mg_workers_harness.cpp — the worker hand-off of libcutensorMg.so (csrc/mg/mg_workers.h) on its own: four workers with a no-op start
// callable, a few thousand run() / wait() rounds whose callables live on a frame that is left right after wait(), one round in which a
// worker reports a failure, an idle gap long enough for the workers to go to sleep and be woken again, and shutdown().  Built plain and
// with -fsanitize=thread by tests/test_mg_workers_cpu.py; exit status 0 and nothing on stderr is a pass.
#include <chrono>
#include <cstdio>
#include <thread>

#include "../../cudalibrarysamples_amd/csrc/mg/mg_workers.h"

namespace {

constexpr int kWorkers = 4;

// One round: every worker adds its index + 1 to its own slot and to a shared sum; the callable and everything it captures live on this
// frame, which is left right after wait() — what cutensorMgContraction's phases do.
int one_round(MgWorkers& w, int round, int failingWorker, long long* total) {
    long long slot[kWorkers] = {0, 0, 0, 0};
    std::atomic<long long> sum{0};
    const MgWorkers::Phase fn = [&](int g) -> int {
        slot[g] += g + 1 + round;
        sum.fetch_add(g + 1, std::memory_order_relaxed);
        return g == failingWorker ? 7 : 0;
    };
    w.run(fn);
    const int st = w.wait();
    for (int g = 0; g < kWorkers; ++g)
        if (slot[g] != g + 1 + round) { std::fprintf(stderr, "round %d: worker %d did not run exactly once\n", round, g); return -1; }
    if (sum.load() != kWorkers * (kWorkers + 1) / 2) { std::fprintf(stderr, "round %d: wrong sum\n", round); return -1; }
    *total += sum.load();
    return st;
}

}  // namespace

int main() {
    MgWorkers w;
    std::atomic<int> started{0};
    w.start(kWorkers, [&](int) { started.fetch_add(1); });
    if (!w.active()) { std::fprintf(stderr, "no workers\n"); return 1; }
    long long total = 0;
    const int rounds = 3000;
    for (int r = 0; r < rounds; ++r) {
        // an idle gap: the workers spin for a few microseconds' worth of pauses, then sleep on the condition variable and must wake up
        if (r == 1000 || r == 2000) std::this_thread::sleep_for(std::chrono::milliseconds(30));
        const int failing = r == 1500 ? 2 : -1;
        const int st = one_round(w, r, failing, &total);
        if (st != (failing >= 0 ? 7 : 0)) { std::fprintf(stderr, "round %d: status %d\n", r, st); return 1; }
    }
    w.shutdown();
    if (w.active() || started.load() != kWorkers) { std::fprintf(stderr, "shutdown left workers, or a start callable did not run\n"); return 1; }
    if (total != (long long)rounds * kWorkers * (kWorkers + 1) / 2) { std::fprintf(stderr, "wrong total\n"); return 1; }
    std::printf("mg workers ok: %d rounds\n", rounds);
    return 0;
}
