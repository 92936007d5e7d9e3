"""Quantized-weight linears for prefill: ``act(x W^T + b)`` with FP8 (``ops.w8.W8Weight``) or MXFP4
(``ops.mx4.MX4Weight``) weights and a tall ``x``.

``kca_wq_gemm`` (csrc/kernels/gemm_wq.hip) is a tiled matrix-core GEMM that converts the weight bytes
in registers: one launch for any M, where the decode kernels behind ``w8_linear`` / ``mx4_linear``
take M > 64 as a loop of 64-row launches that each stream the whole weight again. Its contracts are
the decode kernels': ``w8_linear_reference`` and ``mx4_linear_reference`` -- fp32 accumulation, the FP8
row scale on the sum, bias, activation, one rounding to ``x.dtype`` -- and the same call gives the same
bits (no split-K, no workspace, no atomics).
"""
from __future__ import annotations

import torch

from . import _lib, mx4, w8

MIN_M = w8.MAX_M + 1  # up to 64 rows are one launch of the decode kernels
# The measured crossover above 64 rows (profiles/wq_prefill_ab_r13.jsonl, docs/PERF.md Round 13; bf16, the eight
# GPT-J / NeoX-20B projection shapes, all with K >= 4096). At M = 128 the tiled kernel launches ceil(N / 64)
# workgroups for 256 CUs, and the two-launch slab loop, whose kernels split K over eight waves, is faster where
# those are few: FP8 by 1 - 5 % at 64 and 96 workgroups (N = 4096: 0.95x / 0.99x, N = 6144: 0.95x / 0.98x; 1.02x -
# 1.18x from 192 on), MXFP4 by 13 - 27 % at 64 (N = 4096: 0.87x / 0.73x; N = 6144: 1.37x / 1.55x). At M = 512 the
# tiled kernel wins on every shape (2.1x - 6.3x). Nothing was timed between 128 and 512 rows or below K = 4096 (the
# K split needs a long K to pay): there the tiled kernel runs.
SLAB_MAX_M = 128
SLAB_MIN_K = 4096
SLAB_MAX_WORKGROUPS = {0: 96, 1: 64}  # by fmt (0 FP8, 1 MXFP4): ceil(N / 64) up to which the slab loop wins


def takes_slab_loop(M: int, N: int, K: int, fmt: int) -> bool:
    """True where ``wq_linear`` hands a tall input to the slab loop (the crossover above)."""
    return MIN_M <= M <= SLAB_MAX_M and K >= SLAB_MIN_K and -(-N // 64) <= SLAB_MAX_WORKGROUPS[fmt]


def wq_linear(x: torch.Tensor, w, bias: torch.Tensor | None = None, act: int = 0,
              out: torch.Tensor | None = None, dispatch: bool = True) -> torch.Tensor:
    """``act(x W^T + b)`` for a ``W8Weight`` or an ``MX4Weight``. x [M, K] bf16 / fp16 on the GPU with
    M > 64 and the layout the weight's own op asks for (unit column stride, 16-byte-aligned rows, a
    contiguous bias of ``x.dtype``) is ONE ``kca_wq_gemm`` launch; M <= 64, and the few-workgroup shapes at
    M <= 128 where the slab loop measured faster (``takes_slab_loop``), are ``w8_linear`` / ``mx4_linear``;
    anything else -- CPU tensors, fp32, odd strides -- the reference path. ``dispatch=False``: the tiled kernel
    whatever M (benchmarks, tests). ``act``: 0 none, 1 tanh GELU, 2 erf GELU (``ops.gemv.ACT``)."""
    if isinstance(w, w8.W8Weight):
        mod, fmt, small, ref = w8, 0, w8.w8_linear, w8.w8_linear_reference
    elif isinstance(w, mx4.MX4Weight):
        mod, fmt, small, ref = mx4, 1, mx4.mx4_linear, mx4.mx4_linear_reference
    else:
        raise TypeError(f"wq_linear: expected a W8Weight or an MX4Weight, got {type(w).__name__}")
    M, K = x.shape
    N = w.shape[0]
    if K != w.shape[1]:
        raise ValueError(f"wq_linear: x has K = {K}, the weight {w.shape[1]}")
    if dispatch and (M < MIN_M or takes_slab_loop(M, N, K, fmt)):
        return small(x, w, bias, act, out=out)
    if x.is_cuda and w.q.is_cuda and M > 0 and mod._native_ok(x, w, bias, out):
        if not _lib.has("kca_wq_gemm"):  # a GPU tensor never falls back because the kernel is missing
            _lib.require()
            raise RuntimeError("kca_wq_gemm missing from the kernel library (rebuild: python tools/build_ext.py)")
        y = out if out is not None else torch.empty(M, N, device=x.device, dtype=x.dtype)
        dt = 0 if x.dtype == torch.bfloat16 else 1
        rc = _lib.call_rc("kca_wq_gemm", x.data_ptr(), x.stride(0), w.q.data_ptr(), w.scale.data_ptr(),
                          _lib.ptr(bias), y.data_ptr(), y.stride(0), M, N, K, int(act), dt, fmt, _lib.stream())
        if rc == 0:
            return y
    y = ref(x, w, bias, act)
    if out is not None:
        out.copy_(y)
        return out
    return y


__all__ = ["wq_linear", "takes_slab_loop", "MIN_M", "SLAB_MAX_M", "SLAB_MIN_K", "SLAB_MAX_WORKGROUPS"]
