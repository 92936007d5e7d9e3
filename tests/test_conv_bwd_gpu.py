"""The native 3x3 convolution backward (ops/conv.py, csrc/kernels/conv_igemm_bwd.hip) against the fp32
``aten.convolution_backward``: the weight flip (a pure permutation), the data gradient through the
forward kernel, the split-K weight gradient (automatic, forced, uneven splits, run-to-run bits), and the
autograd dispatch behind ``_BWD_MODE``. Shapes: blocks spanning two images with every tile row on a
border, H != W, Cout and C of 2.5 tiles."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

# (N, H, W, C, Co)
SHAPES = [(2, 8, 8, 64, 128), (1, 16, 8, 128, 192), (3, 8, 16, 64, 320), (2, 8, 8, 320, 64)]
UNEVEN = (3, 8, 16, 64, 320)  # 6 chunks of 64 pixels: 4 splits are uneven

# Relative Frobenius error allowed: 3 x the error of the fp32 reference rounded to bf16, measured on an
# MI355X at SHAPES: gx 1.616e-3 / 1.653e-3 / 1.665e-3 / 1.650e-3, gw 1.654e-3 / 1.658e-3 / 1.662e-3 /
# 1.657e-3 in the order of SHAPES; the constant is the smallest of them. The margin covers the fp32
# summation order, the only other error source.
REL_MEASURED = 1.616e-3
REL_BOUND = 3 * REL_MEASURED


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs and the fp32 reference of one shape, shared by the tests (never modified)."""
    from kubernetes_cloud_amd.ops import _lib
    from kubernetes_cloud_amd.ops.conv import conv3x3_backward_reference
    _lib.require()
    N, H, W, C, Co = shape
    g = torch.Generator(device=dev).manual_seed(N * 1000 + C + Co)
    x = _cl(torch.randn(N, C, H, W, device=dev, generator=g).bfloat16())
    w = _cl((torch.randn(Co, C, 3, 3, device=dev, generator=g) / (3 * C ** 0.5)).bfloat16())
    b = (0.1 * torch.randn(Co, device=dev, generator=g)).bfloat16()
    gy = _cl(torch.randn(N, Co, H, W, device=dev, generator=g).bfloat16())
    ref = conv3x3_backward_reference(gy, x, w, True, (True, True, True))
    return x, w, b, gy, ref


def _check(got, ref, what, frob=True):
    err = (got.float() - ref).abs().max().item()
    rel = ((got.float() - ref).norm() / ref.norm()).item()
    print(f"{what}: max err {err:.3e} (max|ref| {ref.abs().max().item():.3e}), rel frobenius {rel:.3e}")
    assert err <= 2e-2 * ref.abs().max().item() + 1e-3, (what, err)
    if frob:
        assert rel <= REL_BOUND, (what, rel)


@pytest.mark.parametrize("shape", SHAPES)
def test_flip_weight_native_is_the_permutation(shape):
    from kubernetes_cloud_amd.ops.conv import flip_weight
    w = _case(shape)[1]
    wt = flip_weight(w)
    want = _cl(w.cpu().flip(2, 3).transpose(0, 1))
    assert wt.shape == want.shape and wt.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(wt.cpu(), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad_matches_fp32(shape, monkeypatch):
    from kubernetes_cloud_amd.ops import conv as kconv
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    x, w, b, gy, ref = _case(shape)
    gx = kconv.conv3x3_dgrad(gy, w)
    assert kconv._BWD_STATS == {"dgrad": 1, "wgrad": 0}
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=torch.channels_last)
    _check(gx, ref[0], f"dgrad {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_auto_splits_matches_fp32(shape, monkeypatch):
    from kubernetes_cloud_amd.ops import conv as kconv
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    x, w, b, gy, ref = _case(shape)
    gw = kconv.conv3x3_wgrad(x, gy)
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 1}
    assert gw.shape == w.shape and gw.is_contiguous(memory_format=torch.channels_last)
    _check(gw, ref[1], f"wgrad auto {shape}")


@pytest.mark.parametrize("splits", [1, 2, 4])
def test_wgrad_forced_splits_matches_fp32(splits, monkeypatch):
    from kubernetes_cloud_amd.ops import conv as kconv
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    x, w, b, gy, ref = _case(UNEVEN)
    gw = kconv.conv3x3_wgrad(x, gy, splits=splits)
    assert kconv._BWD_STATS["wgrad"] == 1
    _check(gw, ref[1], f"wgrad S={splits}")


@pytest.mark.parametrize("splits", [1, 4])
def test_wgrad_is_bit_identical_run_to_run(splits):
    from kubernetes_cloud_amd.ops.conv import conv3x3_wgrad
    x, w, b, gy, ref = _case(UNEVEN)
    a_ = conv3x3_wgrad(x, gy, splits=splits)
    b_ = conv3x3_wgrad(x, gy, splits=splits)
    assert torch.equal(a_, b_)


def _autograd(shape, monkeypatch, bwd_mode, need=(True, True, True)):
    from kubernetes_cloud_amd.ops import conv as kconv
    monkeypatch.setattr(kconv, "_MODE", "all")
    monkeypatch.setattr(kconv, "_BWD_MODE", bwd_mode)
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    x, w, b, gy, ref = _case(shape)
    xs, ws_, bs = (t.detach().clone().requires_grad_(n) for t, n in zip((x, w, b), need))
    kconv.conv3x3(xs, ws_, bs).backward(gy)
    return kconv, (xs.grad, ws_.grad, bs.grad), ref


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_autograd_native_backward(shape, monkeypatch):
    kconv, grads, ref = _autograd(shape, monkeypatch, "all")
    assert kconv._BWD_STATS == {"dgrad": 1, "wgrad": 1}
    for g_, r_, what in zip(grads, ref, ("gx", "gw", "gb")):
        _check(g_, r_, f"autograd {what} {shape}", frob=False)


def test_autograd_runs_only_the_products_asked_for(monkeypatch):
    kconv, grads, ref = _autograd(SHAPES[0], monkeypatch, "all", (True, False, False))
    assert kconv._BWD_STATS == {"dgrad": 1, "wgrad": 0}
    assert grads[1] is None and grads[2] is None
    _check(grads[0], ref[0], "only gx", frob=False)
    kconv, grads, ref = _autograd(SHAPES[0], monkeypatch, "all", (False, True, False))
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 1}
    assert grads[0] is None and grads[2] is None
    _check(grads[1], ref[1], "only gw", frob=False)


def test_autograd_default_mode_is_aten(monkeypatch):
    kconv, grads, ref = _autograd(SHAPES[0], monkeypatch, "0")
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 0}
    for g_, r_, what in zip(grads[:2], ref, ("gx", "gw")):  # (aten's own bf16 results, loosely)
        _check(g_, r_, f"aten {what}", frob=False)
    assert grads[2] is not None


def test_mode_1_takes_only_the_measured_shapes(monkeypatch):
    kconv, grads, ref = _autograd(SHAPES[0], monkeypatch, "1")  # a test shape is in neither set
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 0}
    monkeypatch.setattr(kconv, "_FAST_WGRAD", {(8, 8, 64, 128)})
    kconv, grads, ref = _autograd(SHAPES[0], monkeypatch, "1")
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 1}
    for g_, r_, what in zip(grads, ref, ("gx", "gw", "gb")):
        _check(g_, r_, f"mode 1 {what}", frob=False)


def test_unsupported_shape_takes_the_aten_path(monkeypatch):
    """C = 32: neither kernel takes it; the public functions and the dispatch return aten's result."""
    from kubernetes_cloud_amd.ops import conv as kconv
    monkeypatch.setattr(kconv, "_BWD_MODE", "all")
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    g = torch.Generator(device=dev).manual_seed(3)
    x = _cl(torch.randn(2, 32, 8, 8, device=dev, generator=g).bfloat16())
    w = _cl((torch.randn(64, 32, 3, 3, device=dev, generator=g) / 17).bfloat16())
    gy = _cl(torch.randn(2, 64, 8, 8, device=dev, generator=g).bfloat16())
    ref = kconv.conv3x3_backward_reference(gy, x, w, True)
    got = kconv.conv3x3_backward(gy, x, w, [True, True, True])
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 0}
    for g_, r_, what in zip(got[:2], ref, ("gx", "gw")):
        _check(g_, r_, f"C=32 {what}", frob=False)
    assert got[2] is not None and got[2].shape == (64,)
    _check(kconv.conv3x3_dgrad(gy, w), ref[0], "C=32 dgrad fn", frob=False)
    _check(kconv.conv3x3_wgrad(x, gy), ref[1], "C=32 wgrad fn", frob=False)
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 0}
