"""Convenience layer over the ABI for device buffers given as raw pointers.

Everything here is a straight replay of the reference samples' call sequence
(cuTENSOR/contraction.cu:122-265, reduction.cu:96-222, elementwise_permute.cu:100-200): create
descriptors -> operation descriptor -> plan preference -> workspace estimate -> plan -> execute.
PyTorch appears only as the owner of device memory and streams in the callers.
"""
import ctypes

from . import cutensor as ct

_DTYPE_COMPUTE = {ct.R_32F: "32F", ct.R_64F: "64F", ct.R_16F: "16F", ct.R_16BF: "16BF", ct.C_32F: "32F", ct.C_64F: "64F"}


class Handle:
    def __init__(self, plan_cache=0):
        self.h = ctypes.c_void_p()
        ct.check(ct.cutensorCreate(ctypes.byref(self.h)))
        if plan_cache:
            ct.check(ct.cutensorHandleResizePlanCache(self.h, plan_cache))

    def close(self):
        if self.h:
            ct.cutensorDestroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tensor_descriptor(handle, extent, stride=None, dtype=ct.R_32F, alignment=128):
    d = ctypes.c_void_p()
    ct.check(ct.cutensorCreateTensorDescriptor(handle.h, ctypes.byref(d), len(extent), ct.i64(extent),
                                               ct.i64(stride) if stride is not None else None, dtype, alignment))
    return d


class Plan:
    """An operation descriptor + plan pair with its scalar type and workspace requirement."""

    def __init__(self, handle, op, kind, dtype, algo=ct.ALGO_DEFAULT, kernel_rank=0, workspace_limit=None,
                 workspace_pref=ct.WORKSPACE_DEFAULT, autotune=None, cache_mode=None, incremental_count=None, operands_streamed=None):
        self.handle, self.kind, self.dtype = handle, kind, dtype
        self.op = op
        pref = ctypes.c_void_p()
        ct.check(ct.cutensorCreatePlanPreference(handle.h, ctypes.byref(pref), algo, ct.JIT_MODE_NONE))
        for attr, val in ((ct.PLAN_PREFERENCE_KERNEL_RANK, kernel_rank or None), (ct.PLAN_PREFERENCE_AUTOTUNE_MODE, autotune),
                          (ct.PLAN_PREFERENCE_CACHE_MODE, cache_mode), (ct.PLAN_PREFERENCE_INCREMENTAL_COUNT, incremental_count),
                          (ct.AMD_PLAN_PREFERENCE_OPERANDS_STREAMED, (1 if operands_streamed else None))):
            if val is not None:   # contraction_plan_cache.cu:215-237
                v = ctypes.c_int32(val)
                ct.check(ct.cutensorPlanPreferenceSetAttribute(handle.h, pref, attr, ctypes.byref(v), 4))
        est = ctypes.c_uint64(0)
        ct.check(ct.cutensorEstimateWorkspaceSize(handle.h, op, pref, workspace_pref, ctypes.byref(est)))
        self.workspace_estimate = est.value
        limit = est.value if workspace_limit is None else workspace_limit
        self.plan = ctypes.c_void_p()
        st = ct.cutensorCreatePlan(handle.h, ctypes.byref(self.plan), op, pref, limit)
        ct.cutensorDestroyPlanPreference(pref)
        ct.check(st)
        req = ctypes.c_uint64(0)
        ct.check(ct.cutensorPlanGetAttribute(handle.h, self.plan, ct.PLAN_REQUIRED_WORKSPACE, ctypes.byref(req), 8))
        self.required_workspace = req.value
        st_type = ctypes.c_int(0)
        ct.check(ct.cutensorOperationDescriptorGetAttribute(handle.h, op, ct.OPERATION_DESCRIPTOR_SCALAR_TYPE,
                                                            ctypes.byref(st_type), 4))
        self.scalar_type = st_type.value

    def scalar(self, x):
        if self.scalar_type == ct.C_32F:
            return (ctypes.c_float * 2)(complex(x).real, complex(x).imag)
        if self.scalar_type == ct.C_64F:
            return (ctypes.c_double * 2)(complex(x).real, complex(x).imag)
        return ctypes.c_double(x) if self.scalar_type == ct.R_64F else ctypes.c_float(x)

    def describe(self):
        return ct.describe_plan(self.plan)

    def destroy(self):
        if self.plan:
            ct.cutensorDestroyPlan(self.plan)
            self.plan = ctypes.c_void_p()
        if self.op:
            ct.cutensorDestroyOperationDescriptor(self.op)
            self.op = ctypes.c_void_p()

    # ---- execution (raw device pointers as ints) ------------------------------------------------
    def contract(self, alpha, A, B, beta, C, D, workspace=0, workspace_size=0, stream=0):
        a, b = self.scalar(alpha), self.scalar(beta)
        ct.check(ct.cutensorContract(self.handle.h, self.plan, ctypes.byref(a), A, B, ctypes.byref(b), C, D,
                                     workspace or None, workspace_size, stream or None))

    def reduce(self, alpha, A, beta, C, D, workspace=0, workspace_size=0, stream=0):
        a, b = self.scalar(alpha), self.scalar(beta)
        ct.check(ct.cutensorReduce(self.handle.h, self.plan, ctypes.byref(a), A, ctypes.byref(b), C, D,
                                   workspace or None, workspace_size, stream or None))

    def permute(self, alpha, A, B, stream=0):
        a = self.scalar(alpha)
        ct.check(ct.cutensorPermute(self.handle.h, self.plan, ctypes.byref(a), A, B, stream or None))

    def contract_trinary(self, alpha, A, B, C, beta, D, E, workspace=0, workspace_size=0, stream=0):
        a, b = self.scalar(alpha), self.scalar(beta)
        ct.check(ct.cutensorContractTrinary(self.handle.h, self.plan, ctypes.byref(a), A, B, C, ctypes.byref(b), D, E,
                                            workspace or None, workspace_size, stream or None))

    def trinary(self, alpha, A, beta, B, gamma, C, D, stream=0):
        a, b, g = self.scalar(alpha), self.scalar(beta), self.scalar(gamma)
        ct.check(ct.cutensorElementwiseTrinaryExecute(self.handle.h, self.plan, ctypes.byref(a), A, ctypes.byref(b), B,
                                                      ctypes.byref(g), C, D, stream or None))

    def binary(self, alpha, A, gamma, C, D, stream=0):
        a, g = self.scalar(alpha), self.scalar(gamma)
        ct.check(ct.cutensorElementwiseBinaryExecute(self.handle.h, self.plan, ctypes.byref(a), A, ctypes.byref(g),
                                                     C, D, stream or None))


_OPS = {"ADD": ct.OP_ADD, "MUL": ct.OP_MUL, "MAX": ct.OP_MAX, "MIN": ct.OP_MIN}
# per-operand unary operators (opA / opB / opC of the plan helpers below), by name or by cutensorOperator_t value
_UNARY = {"IDENTITY": ct.OP_IDENTITY, "CONJ": ct.OP_CONJ, "SQRT": ct.OP_SQRT, "RELU": ct.OP_RELU, "RCP": ct.OP_RCP, "SIGMOID": ct.OP_SIGMOID,
          "TANH": ct.OP_TANH, "EXP": ct.OP_EXP, "LOG": ct.OP_LOG, "ABS": ct.OP_ABS, "NEG": ct.OP_NEG}


def _unary(op):
    return _UNARY[op.upper()] if isinstance(op, str) else op


def _desc3(handle, specs, dtype, alignment):
    return [tensor_descriptor(handle, e, s, dtype, alignment) for (e, s) in specs]


def _pair_compute(dtype, dtype_out):
    """the compute descriptor of an element-wise plan whose output type may differ from A's (type conversion: bf16 / fp16 <-> fp32 under
    32F, fp32 <-> fp64 under 64F; the library refuses every other pair)"""
    if dtype_out == dtype:
        return _DTYPE_COMPUTE[dtype]
    return "64F" if ct.R_64F in (dtype, dtype_out) else "32F"


def _typed_value(value, dtype):
    """one real value in the storage format of dtype (CUTENSOR_OPERATION_DESCRIPTOR_PADDING_VALUE is read in the output's type)"""
    import struct
    if dtype == ct.R_64F:
        return ctypes.c_double(value)
    if dtype == ct.R_16F:
        return ctypes.c_uint16(struct.unpack("<H", struct.pack("<e", value))[0])
    if dtype == ct.R_16BF:
        u = struct.unpack("<I", struct.pack("<f", value))[0]
        return ctypes.c_uint16(((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF)      # to nearest even
    return ctypes.c_float(value)


def contraction_plan(handle, extA, modesA, extB, modesB, extC, modesC, dtype=ct.R_32F, strideA=None,
                     strideB=None, strideC=None, strideD=None, compute=None, alignment=128, opA=ct.OP_IDENTITY,
                     opB=ct.OP_IDENTITY, opC=ct.OP_IDENTITY, dtypeA=None, dtypeB=None, **plan_kw):
    """dtypeA / dtypeB: the data type of A / of B where it differs from that of C and D (dtype) — the mixed rows of the type table:
    dtype=ct.C_64F with dtypeA=ct.R_64F or dtypeB=ct.R_64F (a real fp64 operand into a complex128 contraction, compute "64F", complex
    scalars); None: the same type."""
    dA = tensor_descriptor(handle, extA, strideA, dtype if dtypeA is None else dtypeA, alignment)
    dB = tensor_descriptor(handle, extB, strideB, dtype if dtypeB is None else dtypeB, alignment)
    dC = tensor_descriptor(handle, extC, strideC, dtype, alignment)
    dD = tensor_descriptor(handle, extC, strideD, dtype, alignment) if strideD is not None else dC
    op = ctypes.c_void_p()
    st = ct.cutensorCreateContraction(handle.h, ctypes.byref(op), dA, ct.i32(modesA), _unary(opA), dB, ct.i32(modesB),
                                      _unary(opB), dC, ct.i32(modesC), _unary(opC), dD, ct.i32(modesC),
                                      ct.compute_desc(compute or _DTYPE_COMPUTE[dtype]))
    for d in {id(x): x for x in (dA, dB, dC, dD)}.values():
        ct.cutensorDestroyTensorDescriptor(d)
    ct.check(st)
    return Plan(handle, op, "contraction", dtype, **plan_kw)


def reduction_plan(handle, extA, modesA, extC, modesC, dtype=ct.R_32F, strideA=None, strideC=None,
                   op_reduce=ct.OP_ADD, compute=None, alignment=128, opA=ct.OP_IDENTITY, opC=ct.OP_IDENTITY, **plan_kw):
    dA, dC = _desc3(handle, [(extA, strideA), (extC, strideC)], dtype, alignment)
    op = ctypes.c_void_p()
    st = ct.cutensorCreateReduction(handle.h, ctypes.byref(op), dA, ct.i32(modesA), _unary(opA), dC, ct.i32(modesC),
                                    _unary(opC), dC, ct.i32(modesC), op_reduce,
                                    ct.compute_desc(compute or _DTYPE_COMPUTE[dtype]))
    ct.cutensorDestroyTensorDescriptor(dA)
    ct.cutensorDestroyTensorDescriptor(dC)
    ct.check(st)
    return Plan(handle, op, "reduction", dtype, **plan_kw)


def permutation_plan(handle, extA, modesA, extB, modesB, dtype=ct.R_32F, strideA=None, strideB=None,
                     compute=None, alignment=128, padding=None, opA=ct.OP_IDENTITY, dtypeB=None, **plan_kw):
    """padding = (left[], right[], value): CUTENSOR_OPERATION_DESCRIPTOR_PADDING_* per output mode
    (elementwise_permute_padding.cu:178-195); the output buffer then holds extB + left + right per mode.
    dtypeB: the output's data type where it differs from A's (dtype) — a converting permutation; None: the same type."""
    dtypeB = dtype if dtypeB is None else dtypeB
    dA = tensor_descriptor(handle, extA, strideA, dtype, alignment)
    dB = tensor_descriptor(handle, extB, strideB, dtypeB, alignment)
    op = ctypes.c_void_p()
    st = ct.cutensorCreatePermutation(handle.h, ctypes.byref(op), dA, ct.i32(modesA), _unary(opA), dB, ct.i32(modesB),
                                      ct.compute_desc(compute or _pair_compute(dtype, dtypeB)))
    ct.cutensorDestroyTensorDescriptor(dA)
    ct.cutensorDestroyTensorDescriptor(dB)
    ct.check(st)
    if padding is not None:
        left, right, value = padding
        n = len(extB)
        l = (ctypes.c_int32 * n)(*left)
        r = (ctypes.c_int32 * n)(*right)
        ct.check(ct.cutensorOperationDescriptorSetAttribute(handle.h, op, 4, l, 4 * n))    # PADDING_LEFT
        ct.check(ct.cutensorOperationDescriptorSetAttribute(handle.h, op, 5, r, 4 * n))    # PADDING_RIGHT
        if value is not None:          # (None: the descriptor's default, zero)
            # bytes: the value as the caller laid it out, passed through as it is; else one real value in the output's storage format
            v = (ctypes.c_char * len(value)).from_buffer_copy(value) if isinstance(value, (bytes, bytearray)) else _typed_value(value, dtypeB)
            ct.check(ct.cutensorOperationDescriptorSetAttribute(handle.h, op, 6, ctypes.byref(v), ctypes.sizeof(v)))   # PADDING_VALUE
    plan_kw.setdefault("workspace_limit", 0)   # elementwise_permute.cu:183-187
    return Plan(handle, op, "permutation", dtype, **plan_kw)


def binary_plan(handle, extA, modesA, extC, modesC, op="ADD", dtype=ct.R_32F, compute=None, alignment=128, opA=ct.OP_IDENTITY,
                opC=ct.OP_IDENTITY, strideA=None, strideC=None, dtypeC=None, **plan_kw):
    """D = op(alpha * opA(perm(A)), gamma * opC(C)) — cutensorCreateElementwiseBinary (elementwise_binary.cu:149-153); opA / opC: a unary
    operator by value or by name ("ABS", "RELU", ...).  dtypeC: the data type of C and D where it differs from A's (dtype) — a
    converting plan; None: the same type."""
    dtypeC = dtype if dtypeC is None else dtypeC
    dA = tensor_descriptor(handle, extA, strideA, dtype, alignment)
    dC = tensor_descriptor(handle, extC, strideC, dtypeC, alignment)
    opd = ctypes.c_void_p()
    st = ct.cutensorCreateElementwiseBinary(handle.h, ctypes.byref(opd), dA, ct.i32(modesA), _unary(opA), dC, ct.i32(modesC),
                                            _unary(opC), dC, ct.i32(modesC), _OPS[op],
                                            ct.compute_desc(compute or _pair_compute(dtype, dtypeC)))
    ct.cutensorDestroyTensorDescriptor(dA)
    ct.cutensorDestroyTensorDescriptor(dC)
    ct.check(st)
    plan_kw.setdefault("workspace_limit", 0)
    return Plan(handle, opd, "binary", dtype, **plan_kw)


def trinary_plan(handle, extA, modesA, extB, modesB, extC, modesC, extD, modesD, opAB="ADD", opABC="ADD", dtype=ct.R_32F,
                 compute=None, alignment=128, strideA=None, strideB=None, strideC=None, strideD=None, opA=ct.OP_IDENTITY, opB=ct.OP_IDENTITY,
                 opC=ct.OP_IDENTITY, **plan_kw):
    """D = opABC(opAB(alpha * opA(perm(A)), beta * opB(perm(B))), gamma * opC(perm(C))) — cutensorCreateElementwiseTrinary
    (elementwise_trinary.cu:174-182)."""
    dA, dB, dC, dD = _desc3(handle, [(extA, strideA), (extB, strideB), (extC, strideC), (extD, strideD)], dtype, alignment)
    opd = ctypes.c_void_p()
    st = ct.cutensorCreateElementwiseTrinary(handle.h, ctypes.byref(opd), dA, ct.i32(modesA), _unary(opA), dB, ct.i32(modesB),
                                             _unary(opB), dC, ct.i32(modesC), _unary(opC), dD, ct.i32(modesD),
                                             _OPS[opAB], _OPS[opABC], ct.compute_desc(compute or _DTYPE_COMPUTE[dtype]))
    for d in (dA, dB, dC, dD):
        ct.cutensorDestroyTensorDescriptor(d)
    ct.check(st)
    plan_kw.setdefault("workspace_limit", 0)
    return Plan(handle, opd, "trinary", dtype, **plan_kw)


def contraction_trinary_plan(handle, extA, modesA, extB, modesB, extC, modesC, extD, modesD, dtype=ct.R_32F, compute=None,
                             alignment=128, strideA=None, strideB=None, strideC=None, strideD=None, strideE=None, opA=ct.OP_IDENTITY,
                             opB=ct.OP_IDENTITY, opC=ct.OP_IDENTITY, opD=ct.OP_IDENTITY, **plan_kw):
    """E = alpha * opA(A) * opB(B) * opC(C) + beta * opD(D) — cutensorCreateContractionTrinary (contraction_trinary.cu:191-198); E shares
    D's descriptor as in the sample unless strideE gives it pitches of its own (same extents and modes)."""
    dA, dB, dC, dD = _desc3(handle, [(extA, strideA), (extB, strideB), (extC, strideC), (extD, strideD)], dtype, alignment)
    dE = tensor_descriptor(handle, extD, strideE, dtype, alignment) if strideE is not None else dD
    opd = ctypes.c_void_p()
    st = ct.cutensorCreateContractionTrinary(handle.h, ctypes.byref(opd), dA, ct.i32(modesA), _unary(opA), dB, ct.i32(modesB),
                                             _unary(opB), dC, ct.i32(modesC), _unary(opC), dD, ct.i32(modesD), _unary(opD),
                                             dE, ct.i32(modesD), ct.compute_desc(compute or _DTYPE_COMPUTE[dtype]))
    for d in {id(x): x for x in (dA, dB, dC, dD, dE)}.values():
        ct.cutensorDestroyTensorDescriptor(d)
    ct.check(st)
    return Plan(handle, opd, "contraction_trinary", dtype, **plan_kw)


def blocksparse_plan(handle, sections, modes, blocks, dtype=ct.R_64F, compute=None, strides=(None, None, None), **plan_kw):
    """D = alpha * A * B + beta * C over blocks — cutensorCreateBlockSparseTensorDescriptor / cutensorCreateBlockSparseContraction
    (blocksparse.cu:102-107, :177-182).  sections: mode -> the extents of its sections; modes = (modesA, modesB, modesC); blocks = per
    tensor the section coordinates of its stored blocks; strides: per tensor None (packed blocks) or one stride list per block.  C and D
    share one descriptor as in the sample."""
    descs = []
    for m, coords, st in zip(modes, blocks, strides):
        d = ctypes.c_void_p()
        ct.check(ct.cutensorCreateBlockSparseTensorDescriptor(
            handle.h, ctypes.byref(d), len(m), len(coords), (ctypes.c_uint32 * len(m))(*[len(sections[c]) for c in m]),
            ct.i64([e for c in m for e in sections[c]]), ct.i32([x for c in coords for x in c]),
            ct.i64([x for blk in st for x in blk]) if st is not None else None, dtype))
        descs.append(d)
    op = ctypes.c_void_p()
    mA, mB, mC = modes
    st = ct.cutensorCreateBlockSparseContraction(handle.h, ctypes.byref(op), descs[0], ct.i32(mA), ct.OP_IDENTITY, descs[1], ct.i32(mB),
                                                 ct.OP_IDENTITY, descs[2], ct.i32(mC), ct.OP_IDENTITY, descs[2], ct.i32(mC),
                                                 ct.compute_desc(compute or ("64F" if dtype == ct.R_64F else "32F")))
    for d in descs:
        ct.cutensorDestroyBlockSparseTensorDescriptor(d)
    ct.check(st)
    return Plan(handle, op, "blocksparse", dtype, **plan_kw)
