"""Guarded buffers for the workspace contract (tests/test_gpu_workspace_contract.py) — a helper module, not a conftest.

guarded_workspace(nbytes, fill): a device workspace whose body is EXACTLY nbytes long, at 128 (mod 256) — the alignment the reference
asserts for a workspace (cuTENSOR/contraction.cu:242) and no more — between guards of at least 4 KiB; body and guards are filled with
`fill` (0xFF: a NaN in fp16, bf16, fp32 and fp64; 0x00: the other fill), and check() asserts the guards still hold it byte for byte.

guarded_tensor(extents, dtype, pad): an N-mode column-major tensor (first mode fastest) whose first mode's pitch is padded by `pad`
elements, inside a NaN-filled buffer with 4 KiB of guard on each side — D for every family, C where it has a layout of its own.
check_guard() asserts that every byte outside the tensor's own elements is still 0xFF.

reference(): the case in fp64 / complex128 by torch.einsum on the rounded inputs; TOL: the tolerances the family tests use."""
import numpy as np
import torch

GUARD = 4096

TORCH_DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32, "float64": torch.float64,
                "complex64": torch.complex64, "complex128": torch.complex128}

# (rtol, atol as a fraction of max |reference|, absolute atol): fp32 rtol 1e-4 with atol 1e-4 x max |ref| (tests/test_gpu_repack.py: data
# of both signs cancels), the 16-bit ones of tests/test_gpu_h16_unaligned.py exactly (bf16 8e-3 / 3e-2, fp16 2e-3 / 1e-2), fp64 1e-12,
# complex64 1e-5, complex128 1e-12 (each with the fp32 form of atol)
TOL = {"float32": (1e-4, 1e-4, 0.0), "bfloat16": (8e-3, 0.0, 3e-2), "float16": (2e-3, 0.0, 1e-2), "float64": (1e-12, 1e-12, 0.0),
       "complex64": (1e-5, 1e-5, 0.0), "complex128": (1e-12, 1e-12, 0.0)}


def wide(dtype_name):
    return torch.complex128 if TORCH_DTYPES[dtype_name].is_complex else torch.float64


class GuardedWorkspace:
    def __init__(self, nbytes, fill, device="cuda"):
        self.nbytes, self.fill = int(nbytes), int(fill)
        self.buf = torch.full((2 * GUARD + 512 + self.nbytes,), self.fill, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.offset = GUARD + (128 - (base + GUARD)) % 256           # body at 128 (mod 256), at least GUARD bytes in
        assert (base + self.offset) % 256 == 128 and self.buf.numel() - self.offset - self.nbytes >= GUARD
        self.ptr = base + self.offset

    def refill(self, fill):
        self.fill = int(fill)
        self.buf.fill_(self.fill)

    def check(self, what=""):
        host = self.buf.cpu().numpy()
        body_end = self.offset + self.nbytes
        bad = np.flatnonzero(np.concatenate([host[:self.offset], host[body_end:]]) != self.fill)
        if bad.size:
            first = int(bad[0])
            if first < self.offset:
                where = "%d bytes before the body" % (self.offset - first)
            else:
                where = "%d bytes past the end of the body" % (first - self.offset)
            raise AssertionError("%s: workspace guard overwritten (%d bytes); first at %s (body %d bytes, fill 0x%02x, found 0x%02x)" % (
                what, bad.size, where, self.nbytes, self.fill, host[first if first < self.offset else first + self.nbytes]))


def guarded_workspace(nbytes, fill):
    return GuardedWorkspace(nbytes, fill)


def packed_strides(extents, pad=0):
    s, run = [], 1
    for i, e in enumerate(extents):
        s.append(run)
        run *= (e + pad) if i == 0 else e
    return s


class GuardedTensor:
    """extents (column-major, first fastest), strides with the first mode's pitch padded by `pad` elements, NaN everywhere else."""

    def __init__(self, extents, dtype_name, pad=0, device="cuda"):
        self.extents, self.dtype_name = list(extents), dtype_name
        self.tdt = TORCH_DTYPES[dtype_name]
        self.es = torch.empty((), dtype=self.tdt).element_size()
        self.strides = packed_strides(self.extents, pad)
        span = 1 + sum((e - 1) * s for e, s in zip(self.extents, self.strides)) if self.extents else 1
        self.g = GUARD // self.es
        self.raw = torch.full(((2 * self.g + span) * self.es,), 0xFF, dtype=torch.uint8, device=device)
        self.buf = self.raw.view(self.tdt)
        self.ptr = self.buf.data_ptr() + self.g * self.es
        assert self.ptr % 256 == 0
        # the elements of the tensor, as a boolean mask over buf
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool)
        mask.as_strided(self._rev(self.extents), self._rev(self.strides), self.g).fill_(True)
        self.mask = mask

    @staticmethod
    def _rev(x):
        return list(reversed(x)) or [1]

    def view(self, buf=None):
        """the logical tensor (modes in descriptor order) over buf (default: the device buffer)"""
        b = self.buf if buf is None else buf
        v = b.as_strided(self._rev(self.extents), self._rev(self.strides), self.g)
        return v.permute(*reversed(range(v.dim()))) if self.extents else v.reshape(())

    def refill_nan(self):
        self.raw.fill_(0xFF)

    def set(self, host):
        """write the logical host tensor into the elements (the padding stays NaN)"""
        self.view().copy_(host.to(self.buf.device))

    def get(self):
        return self.view(self.buf.cpu()).clone()

    def check_guard(self, what=""):
        host = self.raw.cpu().numpy().reshape(-1, self.es)
        outside = ~self.mask.numpy()
        bad = np.flatnonzero(outside & (host != 0xFF).any(axis=1))
        if bad.size:
            first = int(bad[0])
            raise AssertionError("%s: %d elements outside D (padding or guard) written; first at element %d of the buffer (tensor starts at %d)" % (
                what, bad.size, first, self.g))

    def bits(self):
        return self.raw.cpu().numpy().copy()


def guarded_tensor(extents, dtype_name, pad=0):
    return GuardedTensor(extents, dtype_name, pad)


def packed_device(host):
    """a logical host tensor (modes in descriptor order) -> packed column-major device buffer"""
    return host.permute(*reversed(range(host.dim()))).contiguous().cuda() if host.dim() else host.reshape(1).cuda()


def random_tensor(extents, dtype_name, gen, lo=-1.0, hi=1.0):
    """U(lo, hi) drawn in fp64 and rounded once to the data type (complex: both parts), as a logical CPU tensor"""
    tdt = TORCH_DTYPES[dtype_name]
    def draw():
        return torch.rand(list(extents), generator=gen, dtype=torch.float64) * (hi - lo) + lo
    x = torch.complex(draw(), draw()) if tdt.is_complex else draw()
    return x.to(tdt)


def reference(eq, *operands, dtype_name):
    w = wide(dtype_name)
    return torch.einsum(eq, *[o.to(w) for o in operands])


def assert_close(got, ref, dtype_name, what=""):
    rtol, frac, atol_abs = TOL[dtype_name]
    got64, ref64 = got.to(ref.dtype), ref
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    err = (got64 - ref64).abs()
    tol = atol_abs + frac * scale + rtol * ref64.abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.argmax((err - tol).reshape(-1)))
        raise AssertionError("%s: %d/%d elements off; worst flat index %d: got %r ref %r (rtol %g)" % (
            what, int(bad.sum()), bad.numel(), i, got64.reshape(-1)[i].item(), ref64.reshape(-1)[i].item(), rtol))
