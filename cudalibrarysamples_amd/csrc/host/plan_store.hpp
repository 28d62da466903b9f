// plan_store.hpp — the tuning state behind a handle, with one owner: the per-problem plan cache (what the cache FILE holds), the plan
// memo, incremental autotuning's trial state and the event pairs of trials that were not read yet.  Everything else in the library
// talks to it through PlanStore's member functions; its maps, its capacity and its mutex are private.
#pragma once
#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include <cutensor.h>

#define CTAMD_HIDDEN __attribute__((visibility("hidden")))   // internal to libcutensor.so: not an exported symbol

struct PlanCacheEntry {
    std::string key;
    int         kernel;
    uint32_t    splitK;
};

// Plan memo: the einsum.cu flow creates descriptors and a plan inside every call (einsum.cu:264-329) with the plan cache on
// (:443-445), so a repeated problem must cost a lookup, not a planning pass.  The key is a fixed-size POD built straight from
// the operation descriptor + preference + workspace limit (no strings, no allocation); the value is a finished prototype plan
// that a hit clones.  Problems with more than kMaxModes mode slots in total are simply not memoised.
struct PlanMemoKey {
    static constexpr int kMaxModes = 40;          // sum of the mode counts of A, B, C, D
    uint64_t wsLimit = 0;
    int32_t  algo = 0, kernelRank = 0, autotune = 0, incrementalCount = 0;
    uint32_t alignment[4] = {0, 0, 0, 0};
    uint8_t  kind = 0, dtype = 0, compute = 0, scalarType = 0;
    uint8_t  n[4] = {0, 0, 0, 0};
    uint8_t  op[4] = {0, 0, 0, 0};                 // opA, opB, opC, opReduce
    uint8_t  present = 0, operandsStreamed = 0, dtypeD = 0, dtypeC = 0;   // (dtype above is A's; C's is 255 when there is no C)
    uint32_t used = 0;                             // int64 words of data[] in use
    uint32_t dtypeB = 0;                           // B's type + 1 where it differs from A's (mixed contractions), else 0
                                                   // (no implicit padding anywhere in the head: it is hashed and compared bytewise)
    int64_t  data[3 * kMaxModes];                  // per tensor: modes, extents, strides
    uint64_t hash() const;
    bool operator==(const PlanMemoKey& o) const;
};
struct PlanMemoEntry {
    PlanMemoKey key;
    std::shared_ptr<const cutensorPlan> proto;
    uint64_t stamp = 0;                            // last use, for LRU eviction
};

namespace ctamd {

// the problem signature the per-problem cache is keyed by: the string form is what the cache FILE holds
CTAMD_HIDDEN std::string problem_key(const cutensorOperationDescriptor& op);
// POD memo key: false when the problem is outside what the memo holds
CTAMD_HIDDEN bool build_memo_key(const cutensorOperationDescriptor& op, const cutensorPlanPreference& pr, uint64_t wsLimit, PlanMemoKey& k);

class CTAMD_HIDDEN PlanStore {
public:
    struct Choice { int kernel; uint32_t splitK; };
    struct Stats { uint64_t hits, misses; uint32_t entries; };
    enum class Memo { Off, Miss, Hit };

    PlanStore() = default;
    PlanStore(const PlanStore&) = delete;
    PlanStore& operator=(const PlanStore&) = delete;
    ~PlanStore();   // destroys the event pairs nobody read

    // cutensorHandleResizePlanCache: 0 turns memo and cache off; cache entries are evicted from the smallest key upward, the memo is
    // cleared only when it holds more than n prototypes
    void resize(uint32_t n);
    // the cache file: "cutensor-amd-plancache 1", then one line per problem, key \t kernel \t splitK \t candidates tried \t best time [us]
    cutensorStatus_t write_file(const char* path);                       // (reads the pending measurements first)
    cutensorStatus_t read_file(const char* path, uint32_t* linesRead);   // INSUFFICIENT_WORKSPACE at the first line that does not fit

    // Plan memo.  Off: the capacity is 0 (nothing counted, nothing to insert later); Hit: `proto` is the prototype to clone
    Memo memo_lookup(const PlanMemoKey& key, uint64_t hash, std::shared_ptr<const cutensorPlan>& proto);
    void memo_insert(const PlanMemoKey& key, uint64_t hash, std::shared_ptr<const cutensorPlan> proto);   // evicts the least recently used

    // Per-problem cache.  has_choices: there is an entry at all (a caller builds the string key only then)
    bool has_choices();
    std::optional<Choice> cached_choice(const std::string& key);
    // a measured choice (CUTENSOR_ALGO_DEFAULT_PATIENT), stored only while there is room.  Every write of a cache entry — this one, a
    // trial that beats the best so far (resolve), a line of a cache file — drops the memo: a prototype must never shadow a tuned choice
    void record_choice(const std::string& key, int kernel, uint32_t splitK);

    // Incremental autotuning (contraction_plan_cache.cu:215-237).  next_trial: the rank in 0 .. limit - 1 the next trial plan of the
    // problem takes, nothing once `limit` candidates were tried (or the store is off, or it tunes as many problems as it has room for)
    std::optional<int> next_trial(const std::string& key, int limit);
    // cutensorContract bracketed a trial plan's launches with (e0, e1): the store owns the pair from here and reads it in resolve()
    void add_measurement(const std::string& key, int kernel, uint32_t splitK, hipEvent_t e0, hipEvent_t e1);
    bool has_pending() const { return pendingCount_.load(std::memory_order_relaxed) > 0; }
    void resolve();   // waits for the pending pairs; the fastest candidate seen so far is what the cache holds

    Stats stats();

private:
    // per problem, the candidates tried so far with their measured time; the best one is what the plan cache holds
    struct TuneState {
        int      next = 0;                 // next candidate rank to try
        int      bestKernel = -1;
        uint32_t bestSplitK = 1;
        float    bestMs = 1e30f;
    };
    struct PendingMeasurement { std::string key; int kernel; uint32_t splitK; hipEvent_t e0, e1; };

    bool write_entry(const std::string& key, int kernel, uint32_t splitK, bool overwrite);   // mtx_ held

    std::mutex mtx_;
    uint32_t capacity_ = 64;            // a fresh handle can read a plan-cache file before any resize (contraction_plan_cache.cu:132-152)
    std::map<std::string, PlanCacheEntry> cache_;            // problem signature -> tuned choice
    std::unordered_map<uint64_t, PlanMemoEntry> memo_;       // hashed POD key -> finished prototype plan (at most capacity_)
    uint64_t memoClock_ = 0, memoHits_ = 0, memoMisses_ = 0;
    std::map<std::string, TuneState> tuning_;                // new problems only while it holds fewer than capacity_
    std::vector<PendingMeasurement> pending_;                // trial executions whose events were not read yet
    std::atomic<int> pendingCount_{0};                       // == pending_.size(), readable without the lock
};

}  // namespace ctamd
