// mp_describe.cpp — ctamdMpDescribePlan: everything a plan holds, as one JSON object (tests/test_mp_plan_descriptions_cpu.py compares it
// byte for byte with the plans of the commit that introduced the full description).  The keys and their values are those of the plan
// layout of that commit: offsets of transfers and staging tensors are printed relative to their region, region sizes rounded to 256,
// "stageBytes" of a reduce plan is the offset of the contraction workspace, and a plan prints false / 0 for the algorithm it is not.
#include <cstdio>
#include <cstring>
#include <string>

#include "mp_internal.hpp"

extern "C" int ctamdDescribePlan(const cutensorPlan_t plan, char* buf, size_t len);   // libcutensor.so diagnostic

namespace ctamd_mp CTAMD_MP_HIDDEN {
namespace {

struct Writer {
    std::string j;
    template <typename... T> void add(const char* fmt, T... a) {
        char tmp[256];
        std::snprintf(tmp, sizeof(tmp), fmt, a...);
        j += tmp;
    }
    static const char* tf(bool b) { return b ? "true" : "false"; }
    void ints(const std::vector<int64_t>& v) {
        j += "[";
        for (size_t i = 0; i < v.size(); ++i) add("%s%lld", i ? ", " : "", (long long)v[i]);
        j += "]";
    }
    void box(const Box& b) { j += "["; ints(b.lo); j += ", "; ints(b.hi); j += "]"; }
    void engine_plan(cutensorPlan_t p) {       // ctamdDescribePlan's text of a single-GPU plan, itself a JSON object
        std::vector<char> text(16384);
        j += (p != nullptr && ctamdDescribePlan(p, text.data(), text.size()) > 0) ? text.data() : "null";
    }
    void copy(const CopyOp& c) {
        if (c.plan == nullptr) { j += "null"; return; }
        j += "{\"launches\": [";
        for (size_t i = 0; i < c.launches.size(); ++i) add("%s[%lld, %lld]", i ? ", " : "", (long long)c.launches[i].first, (long long)c.launches[i].second);
        j += "], \"plan\": ";
        engine_plan(c.plan.get());
        j += "}";
    }
    void copies(const std::vector<CopyOp>& v) {
        j += "[";
        for (size_t i = 0; i < v.size(); ++i) { if (i) j += ", "; copy(v[i]); }
        j += "]";
    }
    void transfers(const char* name, const std::vector<Transfer>* v, const GatherPlan* G) {
        j += std::string("\"") + name + "\": [";
        for (size_t i = 0; v != nullptr && i < v->size(); ++i) {
            const Transfer& t = (*v)[i];
            add("%s{\"tensor\": \"%c\", \"src\": %d, \"dst\": %d, \"bytes\": %lld, \"direct\": %s, \"inPlace\": %s, \"launches\": %d",
                i ? ", " : "", t.tensor == 0 ? 'A' : 'B', t.src, t.dst, (long long)t.bytes, tf(t.direct), tf(t.inPlace),
                (int)(t.pack.plan ? t.pack.launches.size() : t.unpack.plan ? t.unpack.launches.size() : 0));
            j += ", \"box\": "; box(t.box);
            add(", \"sendOff\": %lld, \"recvOff\": %lld, \"pack\": ", (long long)(t.pack.plan ? t.sendOff - G->send.off : 0),
                (long long)(t.unpack.plan ? t.recvOff - G->recv.off : 0));
            copy(t.pack);
            j += ", \"unpack\": "; copy(t.unpack);
            j += "}";
        }
        j += "]";
    }
    void gather(const cutensorMpPlan& plan) {
        const GatherPlan& G = *plan.gather;
        j += ", \"operands\": [";
        for (int k = 0; k < 2; ++k) {
            const OperandPlan& o = G.in[k];
            j += k ? ", {\"need\": " : "{\"need\": "; box(o.need);
            add(", \"viewOff\": %lld, \"viewStride\": ", (long long)o.viewOff); ints(o.viewStride);
            add(", \"stageOff\": %lld, \"stageBytes\": %lld, \"localCopies\": ", (long long)(o.stage.bytes ? o.stage.off - G.stage.off : 0),
                (long long)round_up(o.stage.bytes, 256));
            copies(o.localCopies);
            j += "}";
        }
        add("], \"reduce\": null, \"workspace\": {\"send\": %lld, \"recv\": %lld, \"stage\": %lld, \"contraction\": %lld}", (long long)G.send.off,
            (long long)G.recv.off, (long long)G.stage.off, (long long)plan.contractionOff);
    }
    void reduce(const cutensorMpPlan& plan) {
        const ReducePlan& R = *plan.reduce;
        j += ", \"operands\": null, \"reduce\": {";
        add("\"replicatedC\": %s, \"slotElems\": %lld, ", tf(R.replicatedC), (long long)R.slotElems);
        add("\"stage\": [%lld, %lld], \"send\": [%lld, %lld], \"recv\": [%lld, %lld], \"scratch\": [%lld, %lld], ", (long long)R.stage.off,
            (long long)R.stage.bytes, (long long)R.send.off, (long long)R.send.bytes, (long long)R.recv.off, (long long)R.recv.bytes,
            (long long)R.scratch.off, (long long)R.scratch.bytes);
        j += "\"cIn\": "; copy(R.cIn);
        j += ", \"out\": "; copy(R.out);
        j += ", \"pack\": "; copies(R.pack);
        j += ", \"unpack\": "; copy(R.unpack);
        add("}, \"workspace\": {\"stage\": %lld, \"send\": %lld, \"recv\": %lld, \"scratch\": %lld, \"contraction\": %lld}", (long long)R.stage.off,
            (long long)R.send.off, (long long)R.recv.off, (long long)R.scratch.off, (long long)plan.contractionOff);
    }
    void plan(const cutensorMpPlan& p) {
        const GatherPlan* G = p.gather.get();
        const ReducePlan* R = p.reduce.get();
        j = "{";
        add("\"rank\": %d, \"nranks\": %d, \"compute\": %s, ", p.rank, p.nranks, tf(p.compute));
        add("\"algorithm\": \"%s\", \"gatherTotal\": %lld, \"reduceTotal\": %lld, ", R ? "reduce" : "gather", (long long)p.gatherTotal, (long long)p.reduceTotal);
        add("\"reduceDirect\": %s, \"packDirect\": %s, \"recvDirect\": %s, ", tf(R && R->direct), tf(R && R->packDirect), tf(R && R->recvDirect));
        add("\"stagedA\": %s, \"stagedB\": %s, ", tf(G && G->in[0].staged), tf(G && G->in[1].staged));
        add("\"sendBytes\": %lld, \"recvBytes\": %lld, \"stageBytes\": %lld, \"contractionWorkspace\": %llu, \"requiredDevice\": %llu, ",
            (long long)(G ? G->send.bytes : 0), (long long)(G ? G->recv.bytes : 0), (long long)(G ? G->stage.bytes : p.contractionOff),
            (unsigned long long)p.contractionWs, (unsigned long long)p.requiredDevice);
        transfers("sends", G ? &G->sends : nullptr, G);
        j += ", ";
        transfers("recvs", G ? &G->recvs : nullptr, G);
        if (R) reduce(p); else gather(p);
        add(", \"contractionWs\": %llu, \"contraction\": ", (unsigned long long)p.contractionWs);
        engine_plan(p.contraction.get());
        j += "}";
    }
};

}  // namespace
}  // namespace ctamd_mp

extern "C" {

size_t ctamdMpDescribePlan(const cutensorMpPlan_t plan, char* buf, size_t bufSize) try {
    if (plan == nullptr) return 0;
    ctamd_mp::Writer w;
    w.plan(*plan);
    if (buf != nullptr && bufSize > 0) {
        const size_t n = std::min(bufSize - 1, w.j.size());
        std::memcpy(buf, w.j.data(), n);
        buf[n] = 0;
    }
    return w.j.size() + 1;
} CTAMD_API_CATCH_ZERO

}  // extern "C"
