"""3x3 convolution on the matrix cores (``csrc/kernels/conv_igemm.hip``: implicit GEMM over NHWC, no im2col
buffer) for the SD-1.5 UNet / VAE convolutions.

``conv3x3(x, w, bias)`` takes channels-last bf16 tensors (the layout the SD models run in,
``models/unet.py`` ``to_channels_last``): x [N, C, H, W], w [Cout, C, 3, 3] (physically NHWC / KRSC),
stride 1, padding 1. Shapes the kernel does not take (C or Cout not a multiple of 64, N*H*W not a
multiple of 128, other dtypes / layouts, CPU tensors) run ``F.conv2d``.

Backward (``csrc/kernels/conv_igemm_bwd.hip``): the data gradient is the forward kernel on the re-laid
weight ``flip_weight(w)`` (``conv3x3_dgrad``), the weight gradient an MFMA kernel with a deterministic
split-K (``conv3x3_wgrad``), the bias gradient the bf16 column sum of ``ops/linear.py``. Under autograd
they are taken only where ``KCA_CONV_IGEMM_BWD`` allows (default ``0``: PyTorch's
``convolution_backward``, MIOpen, as before); a product whose shape the kernels do not take keeps the
aten call.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib

# "1" (default): the measured shapes below, "all": every supported shape, "0": off (MIOpen everywhere).
# End to end on the same box, KCA_CONV_IGEMM=0 -> 1: txt2img 6.378 / 6.416 -> 6.498 / 6.537 images/s,
# DreamBooth 61.99 / 61.93 -> 62.16 / 62.31 samples/s (profiles/conv_sd_ab_r6.jsonl)
_MODE = os.environ.get("KCA_CONV_IGEMM", "1")
# (H, W, C, Cout) where the kernel (LDS-DMA form) beat the tuned MIOpen solvers in same-box runs
# (profiles/conv_bench_r6.jsonl; UNet at N = 16, VAE decoder at N = 8): UNet 64x64 640 / 960 -> 320 773 /
# 799 vs 625 / 704 TFLOP/s, 320 -> 320 684 vs 642, the 16x16 convs 606-686 vs 524-530; the VAE's 512x512
# convs 871 / 792 vs 766 / 718. MIOpen keeps the UNet's 32x32 convs (606-663 vs 729-784: 320 workgroups
# are 1.25 rounds of the chip), its 8x8 ones (16 blocks) and the VAE's 64-256 px convs (~1 PF there).
_FAST = {(64, 64, 320, 320), (64, 64, 640, 320), (64, 64, 960, 320), (16, 16, 640, 1280), (16, 16, 1280, 1280),
         (16, 16, 2560, 1280), (16, 16, 1920, 1280), (512, 512, 256, 128), (512, 512, 128, 128)}
_VARIANT_SET = False


def supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 4
            and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)):
        return False
    N, C, H, W = x.shape
    Co = w.shape[0]
    return (w.shape[1] == C and C % 64 == 0 and Co % 64 == 0 and (N * H * W) % 128 == 0
            and x.is_contiguous(memory_format=torch.channels_last)
            and w.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and _lib.has("kca_conv3x3_fwd"))


def _fwd(x, w, bias):
    global _VARIANT_SET
    if not _VARIANT_SET:  # A/B: 1 = 128 x 128 tiles, 2 = 256 x 128 tiles (0: by shape)
        _VARIANT_SET = True
        v = int(os.environ.get("KCA_CONV_VARIANT", "0"))
        if v:
            _lib.call("kca_conv3x3_set_variant", v)
    N, C, H, W = x.shape
    Co = w.shape[0]
    y = torch.empty((N, Co, H, W), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    b = bias if bias is not None and bias.dtype == x.dtype and bias.is_contiguous() else None
    _lib.call("kca_conv3x3_fwd", x.data_ptr(), w.data_ptr(), _lib.ptr(b), y.data_ptr(), N, H, W, C, Co,
              _lib.stream())
    if bias is not None and b is None:
        y = y + bias.view(1, -1, 1, 1)
    return y


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return _fwd(x, w, bias)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        return conv3x3_backward(
            gy.contiguous(memory_format=torch.channels_last), x, w,
            [ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]])


# ---- backward ------------------------------------------------------------------------------------

# "0" (default): aten.convolution_backward for all three products, "1": the native data / weight
# gradient on the measured shapes below, "all": on every supported shape.
_BWD_MODE = os.environ.get("KCA_CONV_IGEMM_BWD", "0")
# (H, W, C, Cout) of the forward convolution whose native product's slowest of three timings beat the
# fastest of three tuned-MIOpen timings on the same box (profiles/conv_bwd_bench_r7.jsonl, UNet at N = 16)
# Data gradient (flip included): 0.096-0.44 ms against 0.136-0.53 ms, e.g. 64x64 640 -> 320 0.27 vs 0.40 ms;
# MIOpen keeps 16x16 640 -> 1280 (the forward kernel on 1280 -> 640: 80 workgroups) and the 8x8 convs.
_FAST_DGRAD = {(64, 64, 320, 320), (64, 64, 640, 320), (32, 32, 320, 640), (32, 32, 640, 640), (16, 16, 1280, 1280),
               (16, 16, 2560, 1280), (32, 32, 1280, 640), (64, 64, 960, 320)}
# Weight gradient (reduce included): 0.09-0.59 ms against 0.11-0.59 ms, 8-26 % ahead on the 16x16 / 32x32
# convs, 0.3-7 % on the 64x64 ones (320 channels are 2.5 tiles); MIOpen keeps the 8x8 convs (16 chunks).
_FAST_WGRAD = {(64, 64, 320, 320), (64, 64, 640, 320), (32, 32, 320, 640), (32, 32, 640, 640), (16, 16, 640, 1280),
               (16, 16, 1280, 1280), (16, 16, 2560, 1280), (32, 32, 1280, 640), (64, 64, 960, 320)}
# native launches taken (tests assert which path ran)
_BWD_STATS = {"dgrad": 0, "wgrad": 0}


def _aten_backward(gy, x, w, mask):
    out = torch.ops.aten.convolution_backward(gy, x, w, [w.shape[0]] if mask[2] else None, [1, 1], [1, 1], [1, 1],
                                              False, [0, 0], 1, list(mask))
    return tuple(o if m else None for o, m in zip(out, mask))  # (a backend may fill a product nobody asked for)


def _cl_bf16(t: torch.Tensor) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
            and t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0)


def flip_weight(w: torch.Tensor) -> torch.Tensor:
    """wt [C, Cout, 3, 3] (channels-last) with ``wt[c, co, 2-r, 2-s] = w[co, c, r, s]``: the weight whose
    ``conv3x3`` with the output gradient is the data gradient. Native (``kca_conv3x3_wflip``) for
    channels-last bf16 GPU weights with C and Cout multiples of 64, the formula otherwise."""
    Co, C = w.shape[:2]
    if _cl_bf16(w) and tuple(w.shape[2:]) == (3, 3) and _lib.has("kca_conv3x3_wflip"):
        wt = torch.empty((C, Co, 3, 3), device=w.device, dtype=w.dtype, memory_format=torch.channels_last)
        if _lib.call_rc("kca_conv3x3_wflip", w.data_ptr(), wt.data_ptr(), C, Co, _lib.stream()) == 0:
            return wt
    return w.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)


def _dgrad_native(gy, w):
    """gx, or None where the forward kernel does not take the swapped shape."""
    if not (_cl_bf16(gy) and _cl_bf16(w) and tuple(w.shape[2:]) == (3, 3) and gy.shape[1] == w.shape[0]
            and _lib.has("kca_conv3x3_wflip")):
        return None
    N, Co, H, W = gy.shape
    C = w.shape[1]
    if C % 64 or Co % 64 or (N * H * W) % 128:
        return None
    wt = flip_weight(w)
    gx = torch.empty((N, C, H, W), device=gy.device, dtype=gy.dtype, memory_format=torch.channels_last)
    if _lib.call_rc("kca_conv3x3_fwd", gy.data_ptr(), wt.data_ptr(), None, gx.data_ptr(), N, H, W, Co, C,
                    _lib.stream()) != 0:
        return None
    _BWD_STATS["dgrad"] += 1
    return gx


def _wgrad_native(x, gy, splits=0):
    """gw, or None where ``kca_conv3x3_wgrad`` does not take the shape."""
    if not (_cl_bf16(x) and _cl_bf16(gy) and x.shape[0] == gy.shape[0] and x.shape[2:] == gy.shape[2:]
            and _lib.has("kca_conv3x3_wgrad")):
        return None
    N, C, H, W = x.shape
    Co = gy.shape[1]
    S = splits or _lib.require().kca_conv3x3_wgrad_splits(N, H, W, C, Co)
    if S < 1:
        return None
    gw = torch.empty((Co, C, 3, 3), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    ws = torch.empty((S, Co, 9 * C), device=x.device, dtype=torch.float32) if S > 1 else None
    if _lib.call_rc("kca_conv3x3_wgrad", x.data_ptr(), gy.data_ptr(), gw.data_ptr(), _lib.ptr(ws), N, H, W, C, Co,
                    S, _lib.stream()) != 0:
        return None
    _BWD_STATS["wgrad"] += 1
    return gw


def conv3x3_dgrad(gy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Data gradient of ``conv3x3``: gy [N, Cout, H, W], w [Cout, C, 3, 3] -> gx [N, C, H, W]. Native
    (weight flip + the forward kernel) on supported shapes, ``aten.convolution_backward`` otherwise."""
    gx = _dgrad_native(gy, w)
    if gx is None:
        x = torch.empty((gy.shape[0], w.shape[1]) + tuple(gy.shape[2:]), device=gy.device, dtype=gy.dtype,
                        memory_format=torch.channels_last)
        gx = _aten_backward(gy, x, w, (True, False, False))[0]
    return gx


def conv3x3_wgrad(x: torch.Tensor, gy: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """Weight gradient of ``conv3x3``: x [N, C, H, W], gy [N, Cout, H, W] -> gw [Cout, C, 3, 3]. ``splits``
    forces the split-K count (0: automatic). ``aten.convolution_backward`` on unsupported shapes."""
    gw = _wgrad_native(x, gy, splits)
    if gw is None:
        w = torch.empty((gy.shape[1], x.shape[1], 3, 3), device=x.device, dtype=x.dtype,
                        memory_format=torch.channels_last)
        gw = _aten_backward(gy, x, w, (False, True, False))[1]
    return gw


def _bwd_allowed(fast: set, x, w) -> bool:
    if _BWD_MODE in ("0", "false"):
        return False
    return _BWD_MODE == "all" or (x.shape[2], x.shape[3], x.shape[1], w.shape[0]) in fast


def conv3x3_backward(gy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, mask):
    """(gx, gw, gb) of ``conv3x3`` for the products ``mask`` = [x, w, bias] asks for (None for the
    others). A product is native where ``_BWD_MODE`` allows it and the kernels take the shape; the
    rest is one ``aten.convolution_backward`` call."""
    mask = [bool(m) for m in mask]
    gx = gw = gb = None
    if mask[0] and _bwd_allowed(_FAST_DGRAD, x, w):
        gx = _dgrad_native(gy, w)
    if mask[1] and _bwd_allowed(_FAST_WGRAD, x, w):
        gw = _wgrad_native(x, gy)
    if mask[2] and (gx is not None or gw is not None):
        from .linear import column_sum
        gb = column_sum(gy.permute(0, 2, 3, 1).reshape(-1, gy.shape[1]))
    rest = [mask[0] and gx is None, mask[1] and gw is None, mask[2] and gb is None]
    if any(rest):
        ax, aw, ab = _aten_backward(gy, x, w, rest)
        gx, gw, gb = (ax if rest[0] else gx), (aw if rest[1] else gw), (ab if rest[2] else gb)
    return gx, gw, gb


def conv3x3_backward_reference(gy, x, w, has_bias=False, mask=(True, True, True)):
    """fp32 reference of ``conv3x3_backward``: (gx, gw, gb), None where ``mask`` (or ``has_bias``) is off."""
    m = [bool(mask[0]), bool(mask[1]), bool(has_bias and mask[2])]
    return _aten_backward(gy.float(), x.float(), w.float(), m)


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """stride 1, padding 1 3x3 convolution (see module docstring)."""
    if _MODE in ("0", "false") or not supported(x, w) or \
            (_MODE != "all" and (x.shape[2], x.shape[3], x.shape[1], w.shape[0]) not in _FAST):
        return F.conv2d(x, w, bias, padding=1)
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (bias is not None and bias.requires_grad)):
        return _Conv3x3.apply(x, w, bias)
    return _fwd(x, w, bias)


def conv3x3_reference(x, w, bias=None):
    """fp32 reference of ``conv3x3``."""
    return F.conv2d(x.float(), w.float(), bias.float() if bias is not None else None, padding=1)
