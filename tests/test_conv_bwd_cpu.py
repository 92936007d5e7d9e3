"""CPU side of the 3x3 convolution backward (ops/conv.py): the flipped-weight identity behind the native
data gradient, the fp32 reference's mask / bias handling, and ``conv3x3_backward`` on CPU tensors (the
aten path, no native launch counted)."""
import os

import pytest
import torch


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(N, H, W, C, Co, dtype=torch.float32):
    g = torch.Generator().manual_seed(N * 1000 + C + Co)
    x = _cl(torch.randn(N, C, H, W, generator=g).to(dtype))
    w = _cl((torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dtype))
    gy = _cl(torch.randn(N, Co, H, W, generator=g).to(dtype))
    return x, w, gy


def test_flip_weight_gives_the_data_gradient():
    """H != W and C != Co: an r/s swap or a missing transpose cannot pass."""
    from kubernetes_cloud_amd.ops.conv import conv3x3_backward_reference, conv3x3_reference, flip_weight
    x, w, gy = _inputs(1, 16, 8, 128, 192)
    wt = flip_weight(w)
    assert wt.shape == (128, 192, 3, 3) and wt.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(wt[5, 7, 0, 2], w[7, 5, 2, 0]) and torch.equal(wt[100, 150, 1, 0], w[150, 100, 1, 2])
    got = conv3x3_reference(gy, wt)
    ref = conv3x3_backward_reference(gy, x, w, False, (True, False, False))[0]
    rel = ((got - ref).norm() / ref.norm()).item()
    print("flip identity rel", rel)
    assert rel <= 1e-5
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("mask", [(True, True, True), (True, False, False), (False, True, False),
                                  (False, False, True), (False, True, True)])
@pytest.mark.parametrize("has_bias", [False, True])
def test_backward_reference_honours_mask_and_bias(mask, has_bias):
    from kubernetes_cloud_amd.ops.conv import conv3x3_backward_reference
    x, w, gy = _inputs(2, 4, 6, 8, 16, torch.bfloat16)
    gx, gw, gb = conv3x3_backward_reference(gy, x, w, has_bias, mask)
    xa, wa = x.float().requires_grad_(), w.float().requires_grad_()
    ba = torch.zeros(16, requires_grad=True)
    torch.nn.functional.conv2d(xa, wa, ba, padding=1).backward(gy.float())
    for got, want, on in ((gx, xa.grad, mask[0]), (gw, wa.grad, mask[1]), (gb, ba.grad, mask[2] and has_bias)):
        if not on:
            assert got is None
        else:
            assert got.dtype == torch.float32 and got.shape == want.shape
            assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def test_backward_on_cpu_is_the_reference_and_counts_nothing(monkeypatch):
    from kubernetes_cloud_amd.ops import conv as kconv
    assert kconv._BWD_MODE == os.environ.get("KCA_CONV_IGEMM_BWD", "0")  # off unless the environment asks
    monkeypatch.setattr(kconv, "_BWD_STATS", {"dgrad": 0, "wgrad": 0})
    x, w, gy = _inputs(2, 4, 6, 8, 16)
    for mode in ("0", "all"):  # CPU tensors never take a native product
        monkeypatch.setattr(kconv, "_BWD_MODE", mode)
        for mask in ((True, True, True), (True, False, False), (False, True, False)):
            got = kconv.conv3x3_backward(gy, x, w, mask)
            ref = kconv.conv3x3_backward_reference(gy, x, w, True, mask)
            for g_, r_ in zip(got, ref):
                assert (g_ is None) == (r_ is None)
                if g_ is not None:
                    assert torch.equal(g_, r_)
    assert torch.equal(kconv.conv3x3_dgrad(gy, w), kconv.conv3x3_backward_reference(gy, x, w)[0])
    assert torch.equal(kconv.conv3x3_wgrad(x, gy), kconv.conv3x3_backward_reference(gy, x, w)[1])
    assert kconv._BWD_STATS == {"dgrad": 0, "wgrad": 0}


def test_autograd_default_mode_keeps_stats_zero(monkeypatch):
    """The dispatch defaults: backward off, both measured sets are sets of 4-tuples."""
    from kubernetes_cloud_amd.ops import conv as kconv
    for s in (kconv._FAST_DGRAD, kconv._FAST_WGRAD):
        assert all(len(k) == 4 for k in s)
    monkeypatch.setattr(kconv, "_BWD_MODE", "0")
    x, w, _ = _inputs(1, 4, 4, 8, 8)
    assert not kconv._bwd_allowed(kconv._FAST_DGRAD, x, w) and not kconv._bwd_allowed(kconv._FAST_WGRAD, x, w)
