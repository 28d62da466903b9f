// mp_transport.cpp — the exchange layer of cuTENSORMp: point-to-point groups and the two collectives, over RCCL (one process per GPU)
// and over rank threads of one process on one GPU (the wire of the single-GPU tests).
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <tuple>

#include <rccl/rccl.h>

#include "mp_internal.hpp"

namespace ctamd_mp CTAMD_MP_HIDDEN {

ncclDataType_t nccl_type(hipDataType t) {
    switch (t) {
        case HIP_R_16F: return ncclFloat16;
        case HIP_R_16BF: return ncclBfloat16;
        case HIP_R_64F: return ncclFloat64;
        default: return ncclFloat32;
    }
}

class RcclTransport : public Transport {
public:
    RcclTransport(ncclComm_t c, int r, int n) : comm_(c), rank_(r), size_(n) {}
    int rank() const override { return rank_; }
    int size() const override { return size_; }
    bool begin() override { return ncclGroupStart() == ncclSuccess; }
    bool send(const void* buf, size_t bytes, int peer, hipStream_t s) override {
        return ncclSend(buf, bytes, ncclInt8, peer, comm_, s) == ncclSuccess;
    }
    bool recv(void* buf, size_t bytes, int peer, hipStream_t s) override {
        return ncclRecv(buf, bytes, ncclInt8, peer, comm_, s) == ncclSuccess;
    }
    bool end(hipStream_t) override { return ncclGroupEnd() == ncclSuccess; }
    bool all_reduce(void* buf, size_t count, hipDataType t, void*, hipStream_t s) override {
        return ncclAllReduce(buf, buf, count, nccl_type(t), ncclSum, comm_, s) == ncclSuccess;
    }
    bool reduce_scatter(const void* send, void* recv, size_t countPerRank, hipDataType t, hipStream_t s) override {
        return ncclReduceScatter(send, recv, countPerRank, nccl_type(t), ncclSum, comm_, s) == ncclSuccess;
    }
private:
    ncclComm_t comm_;
    int rank_, size_;
};

// Several ranks as threads of one process on one GPU (see cutensorMp.h).  A send posts {buffer, "data ready" event};
// the matching recv copies device-to-device on the receiver's stream and posts a "consumed" event the sender's
// stream then waits for — the same completion contract as an RCCL send/recv pair.
struct LocalWorld {
    struct Msg { const void* buf; size_t bytes; hipEvent_t ready; hipEvent_t consumed; bool done; };
    int nranks;
    std::mutex mu;
    std::condition_variable cv;
    std::map<std::tuple<int, int, uint64_t>, Msg> box;   // (src, dst, sequence number of the pair)
    std::vector<uint64_t> sendSeq, recvSeq;              // [src * nranks + dst]
    std::vector<const void*> published;                  // collectives: every rank's buffer
    int arrived = 0;
    uint64_t generation = 0;
    explicit LocalWorld(int n) : nranks(n), sendSeq((size_t)n * n, 0), recvSeq((size_t)n * n, 0), published((size_t)n, nullptr) {}
    // host barrier of the rank threads; false when a rank never arrives
    bool barrier(int timeoutS) {
        std::unique_lock<std::mutex> lock(mu);
        const uint64_t gen = generation;
        if (++arrived == nranks) { arrived = 0; ++generation; cv.notify_all(); return true; }
        return cv.wait_for(lock, std::chrono::seconds(timeoutS), [&] { return generation != gen; });
    }
};

class LocalTransport : public Transport {
public:
    LocalTransport(LocalWorld* w, int r) : w_(w), rank_(r) {}
    int rank() const override { return rank_; }
    int size() const override { return w_->nranks; }
    bool begin() override { sent_.clear(); pending_.clear(); return true; }
    bool send(const void* buf, size_t bytes, int peer, hipStream_t s) override {
        LocalWorld::Msg m{buf, bytes, nullptr, nullptr, false};
        if (hipEventCreateWithFlags(&m.ready, hipEventDisableTiming) != hipSuccess) return false;
        if (hipEventRecord(m.ready, s) != hipSuccess) return false;
        std::lock_guard<std::mutex> lock(w_->mu);
        const uint64_t seq = w_->sendSeq[(size_t)rank_ * w_->nranks + peer]++;
        w_->box[std::make_tuple(rank_, peer, seq)] = m;
        sent_.push_back(std::make_tuple(rank_, peer, seq));
        w_->cv.notify_all();
        return true;
    }
    bool recv(void* buf, size_t bytes, int peer, hipStream_t) override {
        pending_.push_back(Pending{buf, bytes, peer});
        return true;
    }
    bool end(hipStream_t s) override {
        bool ok = true;
        for (const Pending& p : pending_) {
            std::unique_lock<std::mutex> lock(w_->mu);
            const uint64_t seq = w_->recvSeq[(size_t)peer_index(p.peer)]++;
            const auto key = std::make_tuple(p.peer, rank_, seq);
            // a peer that never shows up is a usage error (not every rank entered the call): fail, do not hang
            if (!w_->cv.wait_for(lock, std::chrono::seconds(kPeerTimeoutS), [&] { return w_->box.count(key) > 0; })) return false;
            LocalWorld::Msg& m = w_->box[key];
            ok = ok && m.bytes == p.bytes;
            ok = ok && hipStreamWaitEvent(s, m.ready, 0) == hipSuccess;
            ok = ok && hipMemcpyAsync(p.buf, m.buf, std::min(p.bytes, m.bytes), hipMemcpyDeviceToDevice, s) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&m.consumed, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventRecord(m.consumed, s) == hipSuccess;
            m.done = true;
            w_->cv.notify_all();
        }
        for (const auto& key : sent_) {
            std::unique_lock<std::mutex> lock(w_->mu);
            if (!w_->cv.wait_for(lock, std::chrono::seconds(kPeerTimeoutS), [&] { return w_->box[key].done; })) return false;
            LocalWorld::Msg m = w_->box[key];
            w_->box.erase(key);
            lock.unlock();
            if (m.consumed) { ok = ok && hipStreamWaitEvent(s, m.consumed, 0) == hipSuccess; (void)hipEventDestroy(m.consumed); }
            (void)hipEventDestroy(m.ready);
        }
        sent_.clear(); pending_.clear();
        return ok;
    }
    // Collectives: stream-synchronous on purpose (this transport exists for verification, not speed).  Every rank
    // publishes its buffer, sums all of them slot-wise with the engine's own element-wise ADD, and nobody touches a
    // published buffer again before every rank has finished reading it.
    void set_engine(cutensorHandle_t h) override { engine_ = h; }
    bool needs_scratch() const override { return true; }
    bool all_reduce(void* buf, size_t count, hipDataType t, void* scratch, hipStream_t s) override {
        if (!publish(buf, s)) return false;
        bool ok = sum_slots(scratch, 0, count, t, s);
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        ok = w_->barrier(kPeerTimeoutS) && ok;      // every rank has read every buffer
        ok = ok && hipMemcpyAsync(buf, scratch, count * real_size(t), hipMemcpyDeviceToDevice, s) == hipSuccess;
        return ok;
    }
    bool reduce_scatter(const void* send, void* recv, size_t countPerRank, hipDataType t, hipStream_t s) override {
        if (!publish(send, s)) return false;
        bool ok = sum_slots(recv, (size_t)rank_ * countPerRank, countPerRank, t, s);
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        return w_->barrier(kPeerTimeoutS) && ok;
    }
private:
    static constexpr int kPeerTimeoutS = 60;
    static size_t real_size(hipDataType t) { return t == HIP_R_64F ? 8 : (t == HIP_R_32F ? 4 : 2); }
    bool publish(const void* buf, hipStream_t s) {
        if (hipStreamSynchronize(s) != hipSuccess) return false;
        { std::lock_guard<std::mutex> lock(w_->mu); w_->published[(size_t)rank_] = buf; }
        return w_->barrier(kPeerTimeoutS);
    }
    // dst[0..count) = sum over ranks q of published[q][offset .. offset + count)
    bool sum_slots(void* dst, size_t offset, size_t count, hipDataType t, hipStream_t s) {
        const size_t es = real_size(t);
        const int64_t ext[1] = {(int64_t)count};
        const int32_t lab[1] = {0};
        EngineTemps tmp;
        cutensorTensorDescriptor_t& d = tmp.desc[0];
        cutensorPlan_t raw = nullptr;
        cutensorStatus_t st = cutensorCreateTensorDescriptor(engine_, &d, 1, ext, nullptr, t, (uint32_t)es);
        if (st == CUTENSOR_STATUS_SUCCESS)
            st = cutensorCreateElementwiseBinary(engine_, &tmp.op, d, lab, CUTENSOR_OP_IDENTITY, d, lab, CUTENSOR_OP_IDENTITY, d, lab, CUTENSOR_OP_ADD,
                                                 t == HIP_R_64F ? CUTENSOR_COMPUTE_DESC_64F : CUTENSOR_COMPUTE_DESC_32F);
        if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(engine_, &raw, tmp.op, nullptr, 0);
        const EnginePlan plan(raw);
        const void* one = one_of(t);
        bool ok = st == CUTENSOR_STATUS_SUCCESS;
        for (int q = 0; q < w_->nranks && ok; ++q) {
            const char* src = static_cast<const char*>(w_->published[(size_t)q]) + offset * es;
            if (q == 0) ok = hipMemcpyAsync(dst, src, count * es, hipMemcpyDeviceToDevice, s) == hipSuccess;
            else ok = cutensorElementwiseBinaryExecute(engine_, plan.get(), one, src, one, dst, dst, s) == CUTENSOR_STATUS_SUCCESS;
        }
        return ok;
    }
    cutensorHandle_t engine_ = nullptr;
    struct Pending { void* buf; size_t bytes; int peer; };
    size_t peer_index(int peer) const { return (size_t)peer * w_->nranks + rank_; }
    LocalWorld* w_;
    int rank_;
    std::vector<std::tuple<int, int, uint64_t>> sent_;
    std::vector<Pending> pending_;
};

LocalWorld* new_local_world(int nranks) { return new (std::nothrow) LocalWorld(nranks); }
void delete_local_world(LocalWorld* w) { delete w; }
int local_world_size(const LocalWorld* w) { return w->nranks; }
bool rccl_rank_and_size(ncclComm_t comm, int* rank, int* size) {
    return ncclCommUserRank(comm, rank) == ncclSuccess && ncclCommCount(comm, size) == ncclSuccess && *size > 0;
}
Transport* new_rccl_transport(ncclComm_t comm, int rank, int size) { return new (std::nothrow) RcclTransport(comm, rank, size); }
Transport* new_local_transport(LocalWorld* w, int rank) { return new (std::nothrow) LocalTransport(w, rank); }

}  // namespace ctamd_mp
