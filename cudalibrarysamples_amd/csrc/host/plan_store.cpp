// plan_store.cpp — PlanStore (plan_store.hpp): the plan cache with its file, the plan memo and incremental autotuning's state, and the
// two keys they are looked up by.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "internal.hpp"

namespace ctamd {

std::string problem_key(const cutensorOperationDescriptor& op) {
    std::ostringstream ss;
    ss << (int)op.kind << ':' << (int)op.A.desc.dtype << ':' << (op.compute ? op.compute->id : -1);
    // a converting element-wise problem (D's / C's type differs from A's) is another problem than the same-type one of the same shapes
    if ((op.D.present && op.D.desc.dtype != op.A.desc.dtype) || (op.C.present && op.C.desc.dtype != op.A.desc.dtype))
        ss << ":d" << (int)op.D.desc.dtype << ":c" << (op.C.present ? (int)op.C.desc.dtype : -1);
    if (op.B.present && op.B.desc.dtype != op.A.desc.dtype) ss << ":b" << (int)op.B.desc.dtype;      // a mixed fp64 x complex128 contraction
    auto put = [&](const TensorUse& u) {
        ss << '|';
        if (!u.present) return;
        for (size_t i = 0; i < u.modes.size(); ++i)
            ss << u.modes[i] << ',' << u.desc.extent[i] << ',' << u.desc.stride[i] << ';';
        ss << 'a' << u.desc.alignment;
    };
    put(op.A); put(op.B); put(op.C); put(op.D);
    return ss.str();
}

bool build_memo_key(const cutensorOperationDescriptor& op, const cutensorPlanPreference& pr, uint64_t wsLimit, PlanMemoKey& k) {
    if (op.kind != OpKind::Contraction && op.kind != OpKind::Reduction && op.kind != OpKind::Permutation &&
        op.kind != OpKind::ElementwiseBinary) return false;
    if (!op.padLeft.empty() || !op.padRight.empty()) return false;
    const TensorUse* u[4] = {&op.A, &op.B, &op.C, &op.D};
    size_t total = 0;
    for (const TensorUse* t : u) if (t->present) total += t->modes.size();
    if (total > (size_t)PlanMemoKey::kMaxModes) return false;
    k.wsLimit = wsLimit;
    k.algo = (int32_t)pr.algo; k.kernelRank = pr.kernelRank; k.autotune = (int32_t)pr.autotune;
    k.incrementalCount = pr.autotune == CUTENSOR_AUTOTUNE_MODE_INCREMENTAL ? pr.incrementalCount : 0;
    k.operandsStreamed = (uint8_t)(pr.operandsStreamed != 0);
    k.kind = (uint8_t)op.kind; k.dtype = (uint8_t)op.A.desc.dtype; k.compute = (uint8_t)(op.compute ? op.compute->id : 255);
    k.scalarType = (uint8_t)op.scalarType;
    k.dtypeB = (op.B.present && op.B.desc.dtype != op.A.desc.dtype) ? (uint32_t)op.B.desc.dtype + 1u : 0u;
    k.dtypeD = op.D.present ? (uint8_t)op.D.desc.dtype : (uint8_t)255; k.dtypeC = op.C.present ? (uint8_t)op.C.desc.dtype : (uint8_t)255;
    k.op[0] = (uint8_t)op.A.op; k.op[1] = (uint8_t)op.B.op; k.op[2] = (uint8_t)op.C.op; k.op[3] = (uint8_t)op.opReduce;
    k.present = 0;
    uint32_t w = 0;
    for (int i = 0; i < 4; ++i) {
        const TensorUse& t = *u[i];
        k.n[i] = 0; k.alignment[i] = 0;
        if (!t.present) continue;
        k.present |= (uint8_t)(1u << i);
        const size_t n = t.modes.size();
        k.n[i] = (uint8_t)n; k.alignment[i] = t.desc.alignment;
        for (size_t j = 0; j < n; ++j) k.data[w++] = t.modes[j];
        std::memcpy(&k.data[w], t.desc.extent.data(), n * sizeof(int64_t)); w += (uint32_t)n;
        std::memcpy(&k.data[w], t.desc.stride.data(), n * sizeof(int64_t)); w += (uint32_t)n;
    }
    k.used = w;
    return true;
}

}  // namespace ctamd

using namespace ctamd;

uint64_t PlanMemoKey::hash() const {
    // the fixed head (everything before data[]) and the used words, 8 bytes at a time through a multiply-xorshift mix
    auto mix = [](uint64_t h, uint64_t v) { h ^= v; h *= 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); };
    uint64_t h = 0xCBF29CE484222325ull;
    const size_t headWords = offsetof(PlanMemoKey, data) / 8;
    const uint64_t* p = reinterpret_cast<const uint64_t*>(this);
    for (size_t i = 0; i < headWords; ++i) h = mix(h, p[i]);
    for (uint32_t i = 0; i < used; ++i) h = mix(h, (uint64_t)data[i]);
    return h;
}
bool PlanMemoKey::operator==(const PlanMemoKey& o) const {
    return used == o.used && std::memcmp(this, &o, offsetof(PlanMemoKey, data)) == 0 &&
           std::memcmp(data, o.data, (size_t)used * sizeof(int64_t)) == 0;
}

PlanStore::~PlanStore() {
    for (auto& m : pending_) { (void)hipEventDestroy(m.e0); (void)hipEventDestroy(m.e1); }
}

void PlanStore::resize(uint32_t n) {
    std::lock_guard<std::mutex> g(mtx_);
    capacity_ = n;
    while (cache_.size() > n) cache_.erase(cache_.begin());
    if (memo_.size() > n) memo_.clear();
}

// The one place a cache entry is written and the memo dropped with it.  overwrite: an entry of the key is replaced even when the cache
// is full; false when there is no room
bool PlanStore::write_entry(const std::string& key, int kernel, uint32_t splitK, bool overwrite) {
    if (cache_.size() >= capacity_ && !(overwrite && cache_.count(key))) return false;
    cache_[key] = PlanCacheEntry{key, kernel, splitK};
    memo_.clear();
    return true;
}

void PlanStore::record_choice(const std::string& key, int kernel, uint32_t splitK) {
    std::lock_guard<std::mutex> g(mtx_);
    (void)write_entry(key, kernel, splitK, false);
}

bool PlanStore::has_choices() {
    std::lock_guard<std::mutex> g(mtx_);
    return !cache_.empty();
}

std::optional<PlanStore::Choice> PlanStore::cached_choice(const std::string& key) {
    std::lock_guard<std::mutex> g(mtx_);
    auto it = cache_.find(key);
    if (it == cache_.end()) return {};
    return Choice{it->second.kernel, it->second.splitK};
}

PlanStore::Memo PlanStore::memo_lookup(const PlanMemoKey& key, uint64_t hash, std::shared_ptr<const cutensorPlan>& proto) {
    std::lock_guard<std::mutex> g(mtx_);
    if (capacity_ == 0) return Memo::Off;
    auto it = memo_.find(hash);
    if (it == memo_.end() || !(it->second.key == key)) { ++memoMisses_; return Memo::Miss; }
    proto = it->second.proto;
    it->second.stamp = ++memoClock_;
    ++memoHits_;
    return Memo::Hit;
}

void PlanStore::memo_insert(const PlanMemoKey& key, uint64_t hash, std::shared_ptr<const cutensorPlan> proto) {
    std::lock_guard<std::mutex> g(mtx_);
    if (capacity_ == 0) return;
    if (memo_.size() >= capacity_ && memo_.find(hash) == memo_.end()) {
        auto victim = memo_.begin();
        for (auto it = memo_.begin(); it != memo_.end(); ++it)
            if (it->second.stamp < victim->second.stamp) victim = it;
        memo_.erase(victim);
    }
    PlanMemoEntry& e = memo_[hash];
    e.key = key; e.proto = std::move(proto); e.stamp = ++memoClock_;
}

PlanStore::Stats PlanStore::stats() {
    std::lock_guard<std::mutex> g(mtx_);
    return Stats{memoHits_, memoMisses_, (uint32_t)memo_.size()};
}

std::optional<int> PlanStore::next_trial(const std::string& key, int limit) {
    {
        std::lock_guard<std::mutex> g(mtx_);
        if (capacity_ == 0) return {};
    }
    resolve();
    std::lock_guard<std::mutex> g(mtx_);
    auto tit = tuning_.find(key);
    if (tit == tuning_.end() && tuning_.size() < capacity_) tit = tuning_.emplace(key, TuneState{}).first;   // bounded like the cache itself
    if (tit == tuning_.end() || tit->second.next >= limit) return {};
    return tit->second.next++;
}

void PlanStore::add_measurement(const std::string& key, int kernel, uint32_t splitK, hipEvent_t e0, hipEvent_t e1) {
    std::lock_guard<std::mutex> g(mtx_);
    pending_.push_back(PendingMeasurement{key, kernel, splitK, e0, e1});
    pendingCount_.store((int)pending_.size(), std::memory_order_relaxed);
}

// The event pairs are read here — at the next plan creation, before the cache is written — never inside cutensorContract, which stays
// asynchronous; the waiting happens outside the lock.
void PlanStore::resolve() {
    std::vector<PendingMeasurement> todo;
    {
        std::lock_guard<std::mutex> g(mtx_);
        todo.swap(pending_);
        pendingCount_.store(0, std::memory_order_relaxed);
    }
    for (auto& m : todo) {
        float ms = 0.f;
        const bool ok = hipEventSynchronize(m.e1) == hipSuccess && hipEventElapsedTime(&ms, m.e0, m.e1) == hipSuccess;
        (void)hipEventDestroy(m.e0);
        (void)hipEventDestroy(m.e1);
        if (!ok) { (void)hipGetLastError(); continue; }
        std::lock_guard<std::mutex> g(mtx_);
        TuneState& t = tuning_[m.key];
        CT_LOG("incremental autotune: kernel %d splitK %u -> %.3f us (best so far %.3f us)", m.kernel, m.splitK, ms * 1e3, t.bestMs * 1e3);
        if (ms < t.bestMs) {
            t.bestMs = ms; t.bestKernel = m.kernel; t.bestSplitK = m.splitK;
            (void)write_entry(m.key, m.kernel, m.splitK, true);   // (prototypes built from the previous best are stale)
        }
    }
}

cutensorStatus_t PlanStore::write_file(const char* path) {
    resolve();
    std::lock_guard<std::mutex> g(mtx_);
    FILE* f = std::fopen(path, "w");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    std::fprintf(f, "cutensor-amd-plancache 1\n");
    for (const auto& kv : cache_) {   // key, kernel, splitK, candidates tried by incremental autotuning, best time [us]
        auto t = tuning_.find(kv.first);
        const int tried = t != tuning_.end() ? t->second.next : 0;
        const double us = (t != tuning_.end() && t->second.bestMs < 1e29f) ? t->second.bestMs * 1e3 : 0.0;
        std::fprintf(f, "%s\t%d\t%u\t%d\t%.3f\n", kv.second.key.c_str(), kv.second.kernel, kv.second.splitK, tried, us);
    }
    std::fclose(f);
    return CUTENSOR_STATUS_SUCCESS;
}

cutensorStatus_t PlanStore::read_file(const char* path, uint32_t* linesRead) {
    if (linesRead) *linesRead = 0;
    FILE* f = std::fopen(path, "r");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    char header[64];
    int version = 0;
    if (std::fscanf(f, "%63s %d\n", header, &version) != 2 || std::strcmp(header, "cutensor-amd-plancache") != 0) {
        std::fclose(f);
        return CUTENSOR_STATUS_IO_ERROR;
    }
    std::lock_guard<std::mutex> g(mtx_);
    memo_.clear();   // the file may bring a different tuned choice for a memoised problem (dropped also when it brings no line at all)
    std::vector<char> line(1 << 16);
    uint32_t n = 0;
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    while (std::fgets(line.data(), (int)line.size(), f)) {
        char* t1 = std::strchr(line.data(), '\t');
        if (!t1) continue;
        *t1 = 0;
        const std::string key = line.data();
        int kernel = 0, tried = 0;
        unsigned sk = 1;
        double us = 0.0;
        if (std::sscanf(t1 + 1, "%d\t%u\t%d\t%lf", &kernel, &sk, &tried, &us) < 2) continue;
        if (!write_entry(key, kernel, sk, true)) { st = CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE; break; }   // cache too small for the file
        if (tried > 0) {   // resume incremental autotuning where the writing process stopped
            TuneState& t = tuning_[key];
            t.next = tried; t.bestKernel = kernel; t.bestSplitK = sk; t.bestMs = us > 0.0 ? (float)(us * 1e-3) : 1e30f;
        }
        ++n;
    }
    std::fclose(f);
    if (linesRead) *linesRead = n;
    return st;
}
