// mg_workers.h — one worker thread per handle device of libcutensorMg.so (no HIP, no cuTENSOR: plain C++ threads, so the protocol is
// also built and run on its own, tests/harness/mg_workers_harness.cpp).
//
// cutensorMgContraction is driven by ONE host thread (contraction_multi_gpu.cu:286-345), and at 8 devices that thread's enqueue work —
// per device: staging copies, event waits, one or more cutensorContract calls — was measured at 184-195 us per call
// (tools/mg_host_cost_n.py, 8 logical devices), more than the 170 us of device time the sample's 4096^3 leaves each of 8 GPUs.  The
// per-device parts of a call (local staging copies; the pieces' event waits + local contractions + scatters) only touch that device's
// streams, so worker g — which ran `onStart(g)` ONCE (the library: hipSetDevice of its device) — issues them while the calling thread
// keeps everything that orders devices against each other (fork, RCCL groups / peer copies, wave events, join).  A phase is handed out
// with run() and collected with wait(); workers spin briefly for the next phase of a call and sleep on a condition variable between
// calls.  A phase's callable returns 0 or a status; wait() returns the status of a worker that failed, else 0.
//
// The caller's side of the hand-off (enforced in mg_contraction_exec.cpp, WorkerPhases): the callable given to run() outlives the
// phase, every run() is followed by a wait() before anything else leaves the caller's frame, and one caller at a time uses the workers.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

struct __attribute__((visibility("hidden"))) MgWorkers {   // internal to the library that includes it
    using Phase = std::function<int(int)>;
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<uint64_t> phase{0};
    std::atomic<int> pending{0};
    std::atomic<int> failed{0};
    const Phase* fn = nullptr;
    bool stop = false;

    // n workers; worker g calls onStart(g) once, on its own thread, before its first phase
    void start(int n, const std::function<void(int)>& onStart) {
        for (int g = 0; g < n; ++g) {
            threads.emplace_back([this, g, onStart] {
                onStart(g);
                uint64_t seen = 0;
                for (;;) {
                    // a new phase: spin for a while (the next phase of the same call arrives within microseconds), then sleep
                    int spins = 0;
                    while (phase.load(std::memory_order_acquire) == seen && ++spins < 20000) __builtin_ia32_pause();
                    if (phase.load(std::memory_order_acquire) == seen) {
                        std::unique_lock<std::mutex> lk(m);
                        cv.wait(lk, [&] { return stop || phase.load(std::memory_order_acquire) != seen; });
                    }
                    if (phase.load(std::memory_order_acquire) == seen) return;     // stop
                    seen = phase.load(std::memory_order_acquire);
                    int st = -1;
                    try { st = (*fn)(g); } catch (...) { }
                    if (st != 0) failed.store(st, std::memory_order_relaxed);
                    pending.fetch_sub(1, std::memory_order_acq_rel);
                }
            });
        }
    }
    bool active() const { return !threads.empty(); }
    // every worker g runs f(g); returns at once — wait() collects
    void run(const Phase& f) {
        fn = &f;
        failed.store(0, std::memory_order_relaxed);
        pending.store((int)threads.size(), std::memory_order_release);
        {
            std::lock_guard<std::mutex> lk(m);     // pairs with the sleepers' predicate check
            phase.fetch_add(1, std::memory_order_acq_rel);
        }
        cv.notify_all();
    }
    int wait() {
        while (pending.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
        return failed.load(std::memory_order_relaxed);
    }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        for (std::thread& t : threads) t.join();
        threads.clear();
    }
};
