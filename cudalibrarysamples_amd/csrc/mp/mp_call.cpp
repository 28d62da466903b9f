// mp_call.cpp — one cutensorMpContract under either algorithm.  Every workspace offset comes from the plan.
#include "mp_internal.hpp"

namespace ctamd_mp CTAMD_MP_HIDDEN {

namespace {

struct GatherCall {
    cutensorMpHandle* handle;
    const cutensorMpPlan& plan;
    const GatherPlan& G;
    const CallArgs& a;
    hipDataType dtype;
    const void* user[2];
    char* stage(int k) const { return a.ws + G.in[k].stage.off; }
};

// 1. pack what other ranks need from this rank's blocks
cutensorStatus_t pack_sends(const GatherCall& c) {
    for (const Transfer& t : c.G.sends) {
        if (t.direct) continue;
        const cutensorStatus_t st = run_copy(c.handle->h, t.pack, c.dtype, c.user[t.tensor], c.a.ws + t.sendOff, c.handle->stream);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// 2. one group of point-to-point transfers
cutensorStatus_t exchange(const GatherCall& c) {
    if (c.G.sends.empty() && c.G.recvs.empty()) return CUTENSOR_STATUS_SUCCESS;
    Transport& tp = *c.handle->transport;
    hipStream_t s = c.handle->stream;
    if (!tp.begin()) return CUTENSOR_STATUS_EXECUTION_FAILED;
    bool ok = true;
    for (const Transfer& t : c.G.sends)
        ok = ok && tp.send(t.direct ? c.user[t.tensor] : c.a.ws + t.sendOff, (size_t)t.bytes, t.dst, s);
    for (const Transfer& t : c.G.recvs) ok = ok && tp.recv(c.a.ws + t.recvOff, (size_t)t.bytes, t.src, s);
    ok = tp.end(s) && ok;
    return ok ? CUTENSOR_STATUS_SUCCESS : CUTENSOR_STATUS_EXECUTION_FAILED;
}

// 3. assemble the staged operands: the rank's own part, then what arrived in the receive region
cutensorStatus_t assemble(const GatherCall& c) {
    for (int k = 0; k < 2; ++k) {
        const OperandPlan& o = c.G.in[k];
        if (!o.staged) continue;
        for (const CopyOp& copy : o.localCopies) {
            const cutensorStatus_t st = run_copy(c.handle->h, copy, c.dtype, c.user[k], c.stage(k), c.handle->stream);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
        for (const Transfer& t : c.G.recvs) {
            if (t.tensor != k || t.inPlace) continue;
            const cutensorStatus_t st = run_copy(c.handle->h, t.unpack, c.dtype, c.a.ws + t.recvOff, c.stage(k), c.handle->stream);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// 4. the local contraction writes this rank's block of D
cutensorStatus_t contract(const GatherCall& c) {
    const int64_t es = (int64_t)elem_size(c.dtype);
    const void* opnd[2];
    for (int k = 0; k < 2; ++k) {
        const OperandPlan& o = c.G.in[k];
        opnd[k] = o.staged ? static_cast<const void*>(c.stage(k)) : static_cast<const void*>(static_cast<const char*>(c.user[k]) + o.viewOff * es);
    }
    return cutensorContract(c.handle->h, c.plan.contraction.get(), c.a.alpha, opnd[0], opnd[1], c.a.beta, c.a.C ? c.a.C : c.a.D, c.a.D,
                            c.a.ws + c.plan.contractionOff, c.plan.contractionWs, c.handle->stream);
}

bool scalar_is_zero(const void* x, hipDataType t) {
    switch (t) {
        case HIP_R_64F: return *static_cast<const double*>(x) == 0.0;
        case HIP_C_64F: return static_cast<const double*>(x)[0] == 0.0 && static_cast<const double*>(x)[1] == 0.0;
        case HIP_C_32F: return static_cast<const float*>(x)[0] == 0.f && static_cast<const float*>(x)[1] == 0.f;
        default: return *static_cast<const float*>(x) == 0.f;
    }
}

struct ReduceCall {
    cutensorMpHandle* handle;
    const cutensorMpPlan& plan;
    const ReducePlan& R;
    const CallArgs& a;
    const void* C;               // the caller's C, or D when it passed none
    hipDataType dtype;
    bool haveBeta;
    size_t perElem;              // reals per element: the collectives sum reals
    const double zero[2] = {0.0, 0.0};                  // a zero scalar of every scalar type
    cutensorStatus_t contract_into(const void* beta, const void* cIn, void* out) const {
        return cutensorContract(handle->h, plan.contraction.get(), a.alpha, a.A, a.B, beta, cIn, out, a.ws + plan.contractionOff,
                                plan.contractionWs, handle->stream);
    }
};

// replicated C: contract into the partial (the user's D when direct), all-reduce it, copy it out unless direct
cutensorStatus_t reduce_replicated(const ReduceCall& c) {
    const ReducePlan& R = c.R;
    cutensorHandle_t h = c.handle->h;
    hipStream_t s = c.handle->stream;
    char* T = R.direct ? static_cast<char*>(c.a.D) : c.a.ws + R.stage.off;
    const bool mine = c.haveBeta && c.plan.rank == 0;  // beta * C enters the sum once
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    if (!R.direct && mine) { st = run_copy(h, R.cIn, c.dtype, c.C, T, s); if (st != CUTENSOR_STATUS_SUCCESS) return st; }
    st = c.contract_into(mine ? c.a.beta : c.zero, R.direct ? c.C : T, T);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    if (!c.handle->transport->all_reduce(T, (size_t)R.cElems * c.perElem, real_type(c.dtype), c.a.ws + R.scratch.off, s)) return CUTENSOR_STATUS_EXECUTION_FAILED;
    if (!R.direct) st = run_copy(h, R.out, c.dtype, T, c.a.D, s);
    return st;
}

// distributed C: contract into the staged partial, pack the destination blocks into slots, reduce-scatter, unpack the rank's slot
cutensorStatus_t reduce_scattered(const ReduceCall& c) {
    const ReducePlan& R = c.R;
    cutensorHandle_t h = c.handle->h;
    hipStream_t s = c.handle->stream;
    char* P = c.a.ws + R.stage.off;
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    if (c.haveBeta) {
        if (hipMemsetAsync(P, 0, (size_t)R.stage.bytes, s) != hipSuccess) return CUTENSOR_STATUS_EXECUTION_FAILED;
        if (R.cIn.plan != nullptr) { st = run_copy(h, R.cIn, c.dtype, c.C, P, s); if (st != CUTENSOR_STATUS_SUCCESS) return st; }
    }
    st = c.contract_into(c.haveBeta ? c.a.beta : c.zero, P, P);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    const char* send = R.packDirect ? P : c.a.ws + R.send.off;
    for (const CopyOp& copy : R.pack) {
        if (copy.plan == nullptr) continue;
        st = run_copy(h, copy, c.dtype, P, c.a.ws + R.send.off, s);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    char* recv = R.recvDirect ? static_cast<char*>(c.a.D) : c.a.ws + R.recv.off;
    if (!c.handle->transport->reduce_scatter(send, recv, (size_t)R.slotElems * c.perElem, real_type(c.dtype), s)) return CUTENSOR_STATUS_EXECUTION_FAILED;
    if (!R.recvDirect && R.unpack.plan != nullptr) st = run_copy(h, R.unpack, c.dtype, recv, c.a.D, s);
    return st;
}

}  // namespace

cutensorStatus_t run_gather(cutensorMpHandle* handle, const cutensorMpPlan& plan, const CallArgs& a) {
    const GatherCall c{handle, plan, *plan.gather, a, plan.desc.A.dtype, {a.A, a.B}};
    cutensorStatus_t st = pack_sends(c);
    if (st == CUTENSOR_STATUS_SUCCESS) st = exchange(c);
    if (st != CUTENSOR_STATUS_SUCCESS || !plan.compute) return st;
    st = assemble(c);
    return st == CUTENSOR_STATUS_SUCCESS ? contract(c) : st;
}

cutensorStatus_t run_reduce(cutensorMpHandle* handle, const cutensorMpPlan& plan, const CallArgs& a) {
    const hipDataType dt = plan.desc.C.dtype;
    const bool haveBeta = !scalar_is_zero(a.beta, scalar_type(dt, plan.desc.compute));
    const ReduceCall c{handle, plan, *plan.reduce, a, a.C ? a.C : a.D, dt, haveBeta, is_complex(dt) ? 2u : 1u};
    return plan.reduce->replicatedC ? reduce_replicated(c) : reduce_scattered(c);
}

}  // namespace ctamd_mp
