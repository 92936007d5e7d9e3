"""MXFP4 weight-only linears for decode: OCP microscaling FP4, e2m1 elements with one e8m0 scale per
block of 32 consecutive ``k`` of an output row -- 0.53 bytes per weight.

The format (``MX4Weight``), for a weight ``[N, K]`` with ``K % 32 == 0``:

* ``q``: ``[N, K/2]`` uint8. The byte at ``[n, j]`` holds element ``k = 2j`` in its low nibble and
  ``k = 2j + 1`` in its high nibble. A nibble is sign (bit 3), two exponent bits, one mantissa bit;
  the magnitudes by code 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6. Code 0x8 is -0: every consumer treats
  it as zero.
* ``scale``: ``[N, K/32]`` uint8, e8m0: a byte ``E`` means ``2^(E - 127)``. Per block, with ``amax`` the
  largest finite magnitude, ``E - 127 = floor(log2(amax)) - 2`` clamped to [-127, 127] (the OCP rule;
  the exponent is taken exactly with ``frexp``), ``E = 127`` for a block of zeros. 0xFF (NaN) never
  appears.
* elements are ``w / 2^(E - 127)`` formed in fp32, saturated to +-6 and rounded to nearest with ties to
  the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign bit
  follows the input's sign. A non-finite weight counts as 0 (as in ``ops/w8.py``).

``dequantize`` is ``value * 2^(E - 127)`` in fp32: one significant bit pair times a power of two, so it
is exact in bf16 for every scale byte a 16-bit or fp32 weight can produce. In fp16 it is exact only
where ``floor(log2(amax)) >= -21`` (the smallest nonzero element, ``0.5 * 2^(E - 127)``, must reach
fp16's smallest subnormal 2^-24). ``snap_to_grid(w) = dequantize(quantize_weight(w))``; quantizing a
snapped weight gives the same bytes back: a block maximum lands on 4 or 6 times the scale, so the
exponent does not move.

``kca_mx4_gemm`` (csrc/kernels/gemv_mx4.hip) streams the nibbles, converts them in registers
(``v_cvt_scalef32_pk_{bf16,f16}_fp4``) and accumulates in fp32. Its contract is
``mx4_linear_reference``: ``act(sum_k x[m, k] v[n, k] 2^(E[n, k // 32] - 127) + bias[n])`` rounded once
to ``x.dtype``.
"""
from __future__ import annotations

import torch

from . import _lib
from .w8 import _act

BLOCK = 32
MAX_M = 64  # rows per kca_mx4_gemm launch; taller inputs go in slabs
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _exp2_bytes(e: torch.Tensor, dtype) -> torch.Tensor:
    """``2^(E - 127)`` for e8m0 bytes, built from bits (exact; 2^-127 is an fp32 subnormal)."""
    e = e.to(torch.int64)
    if dtype == torch.float64:
        return ((e - 127 + 1023) << 52).view(torch.float64)
    bits = torch.where(e > 0, e << 23, torch.full_like(e, 0x00400000)).to(torch.int32)
    return bits.view(torch.float32).to(dtype)


class MX4Weight:
    """``q``: [N, K/2] uint8, two e2m1 nibbles per byte (low nibble first), contiguous.
    ``scale``: [N, K/32] uint8, e8m0, contiguous."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.uint8 and q.dim() == 2 and q.is_contiguous() and q.shape[1] % (BLOCK // 2) == 0
        assert scale.dtype == torch.uint8 and scale.is_contiguous()
        assert scale.shape == (q.shape[0], q.shape[1] // (BLOCK // 2))
        self.q, self.scale = q, scale

    @property
    def shape(self):
        return torch.Size((self.q.shape[0], 2 * self.q.shape[1]))

    def nbytes(self) -> int:
        return self.q.numel() + self.scale.numel()

    def values(self, dtype=torch.float32) -> torch.Tensor:
        """The e2m1 values (unscaled) as ``dtype``, [N, K]."""
        lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=dtype, device=self.q.device)
        nib = torch.stack((self.q & 0xF, self.q >> 4), dim=2).reshape(self.q.shape[0], -1)
        return lut[nib.long()]

    def scales(self, dtype=torch.float32) -> torch.Tensor:
        """``2^(E - 127)`` per block as ``dtype``, [N, K/32]."""
        return _exp2_bytes(self.scale, dtype)


@torch.no_grad()
def quantize_weight(w: torch.Tensor) -> MX4Weight:
    """The module docstring's rule. Only comparisons, an exact exponent (``frexp``) and a division by a
    power of two: the same bytes on CPU and GPU."""
    if w.dim() != 2 or w.shape[1] % BLOCK or w.shape[1] == 0:
        raise ValueError(f"mx4.quantize_weight: expected [N, K] with K % {BLOCK} == 0, got {tuple(w.shape)}")
    N, K = w.shape
    raw = w.detach().float()
    wf = torch.nan_to_num(raw, nan=0.0, posinf=0.0, neginf=0.0)
    blk = wf.view(N, K // BLOCK, BLOCK)
    amax = blk.abs().amax(dim=2)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex.to(torch.int64) - 3).clamp_(-127, 127) + 127, torch.full_like(ex, 127, dtype=torch.int64))
    a = (blk / _exp2_bytes(e, torch.float32)[:, :, None]).abs_().clamp_(max=6.0)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    sign = torch.signbit(raw).view_as(code) & torch.isfinite(raw).view_as(code)
    code = (code.to(torch.uint8) | (sign.to(torch.uint8) << 3)).view(N, K)
    q = code[:, 0::2] | (code[:, 1::2] << 4)
    return MX4Weight(q.contiguous(), e.to(torch.uint8).contiguous())


def dequantize(w4: MX4Weight, dtype=torch.float32) -> torch.Tensor:
    """``value * 2^(E - 127)`` formed in fp32, then cast."""
    v = w4.values(torch.float32).view(w4.q.shape[0], -1, BLOCK)
    return (v * w4.scales(torch.float32)[:, :, None]).view(w4.q.shape[0], -1).to(dtype)


@torch.no_grad()
def snap_to_grid(w: torch.Tensor) -> torch.Tensor:
    """``w`` moved onto the MXFP4 grid (tests, benchmarks): quantizing the result reproduces its bytes
    and its values exactly (module docstring; the fp16 limit is stated there)."""
    return dequantize(quantize_weight(w)).to(w.dtype)


def mx4_linear_reference(x: torch.Tensor, w4: MX4Weight, bias: torch.Tensor | None = None, act: int = 0,
                         fp64: bool = False) -> torch.Tensor:
    """The kernel's contract in fp32 (fp64 when asked): the scaled e2m1 values against ``x``, bias,
    activation, one rounding to ``x.dtype``."""
    ft = torch.float64 if fp64 else torch.float32
    N = w4.q.shape[0]
    wd = (w4.values(ft).view(N, -1, BLOCK) * w4.scales(ft)[:, :, None]).view(N, -1)
    y = x.to(ft) @ wd.t()
    if bias is not None:
        y = y + bias.to(ft)
    return _act(y, int(act)).to(x.dtype)


def _native_ok(x: torch.Tensor, w4: MX4Weight, bias, out) -> bool:
    K = x.shape[1]
    return (x.dtype in (torch.bfloat16, torch.float16) and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.stride(0) >= K and x.data_ptr() % 16 == 0
            and w4.q.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == x.dtype and bias.is_contiguous() and bias.is_cuda))
            and (out is None or (out.dtype == x.dtype and out.stride(1) == 1 and out.is_cuda)))


def mx4_linear(x: torch.Tensor, w4: MX4Weight, bias: torch.Tensor | None = None, act: int = 0,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """``act(x W^T + b)`` with MXFP4 weights. x [M, K] bf16 / fp16 on the GPU with unit column stride,
    16-byte-aligned rows and a contiguous bias of ``x.dtype`` runs ``kca_mx4_gemm`` (M > 64 in 64-row
    slabs, one launch each); anything else -- CPU tensors, fp32, odd strides -- the reference path.
    ``act``: 0 none, 1 tanh GELU, 2 erf GELU (``ops.gemv.ACT``)."""
    M, K = x.shape
    N = w4.q.shape[0]
    if K != 2 * w4.q.shape[1]:
        raise ValueError(f"mx4_linear: x has K = {K}, the weight {2 * w4.q.shape[1]}")
    if x.is_cuda and w4.q.is_cuda and M > 0 and _native_ok(x, w4, bias, out):
        if not _lib.has("kca_mx4_gemm"):  # a GPU tensor never falls back because the kernel is missing
            _lib.require()
            raise RuntimeError("kca_mx4_gemm missing from the kernel library (rebuild: python tools/build_ext.py)")
        y = out if out is not None else torch.empty(M, N, device=x.device, dtype=x.dtype)
        dt = 0 if x.dtype == torch.bfloat16 else 1
        ok = True
        for m0 in range(0, M, MAX_M):
            xs, ys = x[m0:m0 + MAX_M], y[m0:m0 + MAX_M]
            rc = _lib.call_rc("kca_mx4_gemm", xs.data_ptr(), x.stride(0), w4.q.data_ptr(), w4.scale.data_ptr(),
                              _lib.ptr(bias), ys.data_ptr(), y.stride(0), xs.shape[0], N, K, int(act), dt,
                              _lib.stream())
            if rc != 0:  # (decided by the arguments alone: the first slab refuses or none does)
                ok = False
                break
        if ok:
            return y
    y = mx4_linear_reference(x, w4, bias, act)
    if out is not None:
        out.copy_(y)
        return out
    return y


__all__ = ["MX4Weight", "quantize_weight", "dequantize", "snap_to_grid", "mx4_linear_reference", "mx4_linear",
           "MAX_M", "BLOCK"]
