"""FP8 weight-only linears for decode: e4m3 weights with one fp32 scale per output row.

``quantize_weight`` turns a 16-bit (or fp32) ``[N, K]`` weight into OCP ``e4m3fn`` bytes plus
``scale[n] = absmax(w[n]) / 448``. ``kca_w8_gemm`` (csrc/kernels/gemv_w8.hip) streams those bytes --
half of what the 16-bit decode linears read -- converts them to the activation's type in registers
(exact: every e4m3 value is a bf16 and an fp16 value) and accumulates in fp32. Activations, the KV
cache and the accumulation are untouched; the only error of the scheme is the weight rounding.

The kernel's contract is ``w8_linear_reference``: ``act(scale[n] * sum_k x[m, k] q[n, k] + bias[n])``
-- the scale multiplies the fp32 sum, not the weights -- rounded once to ``x.dtype``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib

E4M3_MAX = 448.0
MAX_M = 64  # rows per kca_w8_gemm launch; taller inputs go in slabs


class W8Weight:
    """``q``: [N, K] uint8, OCP e4m3fn bytes, contiguous. ``scale``: [N] fp32."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.uint8 and q.dim() == 2 and q.is_contiguous()
        assert scale.dtype == torch.float32 and scale.shape == (q.shape[0],)
        self.q, self.scale = q, scale

    @property
    def shape(self):
        return self.q.shape

    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()

    def values(self, dtype=torch.float32) -> torch.Tensor:
        """The e4m3 values (unscaled) as ``dtype``."""
        return self.q.view(torch.float8_e4m3fn).to(dtype)


@torch.no_grad()
def quantize_weight(w: torch.Tensor) -> W8Weight:
    """Per output row: scale = absmax / 448 in fp32 (1 for an all-zero row), q = the fp32 quotient
    clamped to +-448 and rounded to nearest even by torch's ``float8_e4m3fn`` cast. IEEE fp32 division
    and the cast give the same bits on CPU and GPU. The clamp keeps every quotient finite in e4m3, so
    the NaN encodings 0x7F / 0xFF never appear (a non-finite weight is treated as 0)."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight: expected [N, K], got {tuple(w.shape)}")
    wf = torch.nan_to_num(w.detach().float(), nan=0.0, posinf=0.0, neginf=0.0)
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return W8Weight(q.view(torch.uint8).contiguous(), scale.contiguous())


def dequantize(w8: W8Weight, dtype=torch.float32) -> torch.Tensor:
    """``scale[n] * q[n, k]`` formed in fp32, then cast."""
    return (w8.values(torch.float32) * w8.scale[:, None]).to(dtype)


@torch.no_grad()
def snap_to_grid(w: torch.Tensor) -> torch.Tensor:
    """``w`` moved onto a grid that FP8 quantization reproduces exactly (tests, benchmarks): per row
    s = 2^ceil(log2(absmax / 448)), w / s rounded to e4m3 and the row's absmax element forced to +-448,
    so ``quantize_weight`` finds scale == s and the same bytes. Values are (4 significant bits) * 2^k:
    exact in bf16 and fp16."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    s = torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax.clamp_min(1e-30) / E4M3_MAX))),
                    torch.ones_like(amax))
    g = (wf / s[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).float()
    idx = wf.abs().argmax(dim=1, keepdim=True)
    top = torch.where(wf.gather(1, idx) < 0, -E4M3_MAX, E4M3_MAX)
    top = torch.where(amax[:, None] > 0, top, torch.zeros_like(top))
    g.scatter_(1, idx, top)
    return (g * s[:, None]).to(w.dtype)


def _act(y: torch.Tensor, act: int) -> torch.Tensor:
    if act == 1:
        return F.gelu(y, approximate="tanh")
    if act == 2:
        return F.gelu(y)
    return y


def w8_linear_reference(x: torch.Tensor, w8: W8Weight, bias: torch.Tensor | None = None, act: int = 0,
                        fp64: bool = False) -> torch.Tensor:
    """The kernel's contract in fp32 (fp64 when asked): the e4m3 values against ``x``, the row scale on
    the sum, bias, activation, one rounding to ``x.dtype``."""
    ft = torch.float64 if fp64 else torch.float32
    acc = x.to(ft) @ w8.values(ft).t()
    y = acc * w8.scale.to(ft)
    if bias is not None:
        y = y + bias.to(ft)
    return _act(y, int(act)).to(x.dtype)


def _native_ok(x: torch.Tensor, w8: W8Weight, bias, out) -> bool:
    K = x.shape[1]
    return (x.dtype in (torch.bfloat16, torch.float16) and x.stride(1) == 1 and K % 16 == 0 and K >= 16
            and x.stride(0) % 8 == 0 and x.stride(0) >= K and x.data_ptr() % 16 == 0
            and w8.q.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == x.dtype and bias.is_contiguous() and bias.is_cuda))
            and (out is None or (out.dtype == x.dtype and out.stride(1) == 1 and out.is_cuda)))


def w8_linear(x: torch.Tensor, w8: W8Weight, bias: torch.Tensor | None = None, act: int = 0,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """``act(x W^T + b)`` with FP8 weights. x [M, K] bf16 / fp16 on the GPU with unit column stride,
    K % 16 == 0, 16-byte-aligned rows and a contiguous bias of ``x.dtype`` runs ``kca_w8_gemm`` (M > 64
    in 64-row slabs, one launch each); anything else -- CPU tensors, fp32, odd shapes -- the reference
    path. ``act``: 0 none, 1 tanh GELU, 2 erf GELU (``ops.gemv.ACT``)."""
    M, K = x.shape
    N = w8.q.shape[0]
    if K != w8.q.shape[1]:
        raise ValueError(f"w8_linear: x has K = {K}, the weight {w8.q.shape[1]}")
    if x.is_cuda and w8.q.is_cuda and M > 0 and _native_ok(x, w8, bias, out):
        if not _lib.has("kca_w8_gemm"):  # a GPU tensor never falls back because the kernel is missing
            _lib.require()
            raise RuntimeError("kca_w8_gemm missing from the kernel library (rebuild: python tools/build_ext.py)")
        y = out if out is not None else torch.empty(M, N, device=x.device, dtype=x.dtype)
        dt = 0 if x.dtype == torch.bfloat16 else 1
        ok = True
        for m0 in range(0, M, MAX_M):
            xs, ys = x[m0:m0 + MAX_M], y[m0:m0 + MAX_M]
            rc = _lib.call_rc("kca_w8_gemm", xs.data_ptr(), x.stride(0), w8.q.data_ptr(), w8.scale.data_ptr(),
                              _lib.ptr(bias), ys.data_ptr(), y.stride(0), xs.shape[0], N, K, int(act), dt,
                              _lib.stream())
            if rc != 0:  # (decided by the arguments alone: the first slab refuses or none does)
                ok = False
                break
        if ok:
            return y
    y = w8_linear_reference(x, w8, bias, act)
    if out is not None:
        out.copy_(y)
        return out
    return y


__all__ = ["W8Weight", "quantize_weight", "dequantize", "snap_to_grid", "w8_linear_reference", "w8_linear", "MAX_M"]
