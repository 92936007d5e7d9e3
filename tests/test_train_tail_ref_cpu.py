"""The float64 oracles of tests/train_tail_ref.py against independent implementations, and the fp32
CPU fallback of every op inside the bounds tests/test_train_tail_gpu.py applies to the HIP kernels
(same generators, same checks), so a bound that a correct fp32 implementation cannot meet shows
here, without a GPU."""
import math
import struct

import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd import ops
from kubernetes_cloud_amd.train.optim import FlatAdamW

from . import train_tail_ref as R


# ------------------------------------------------------------------------------------ oracle pins
def test_adamw_oracle_matches_torch_adamw_float64():
    torch.manual_seed(0)
    n = 200
    p0 = torch.randn(n, dtype=torch.float64)
    ref = p0.clone().requires_grad_()
    topt = torch.optim.AdamW([ref], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    p, m, v = p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    ones = torch.ones((n + 63) // 64, dtype=torch.uint8)
    for step in range(1, 6):
        g = torch.randn(n, dtype=torch.float64) * step
        ref.grad = g.clone()
        topt.step()
        p, m, v = R.adamw_step64(p, g, m, v, ones, 1.0, 1e-2, (0.9, 0.999), 1e-8, 0.1, step)
        st = topt.state[ref]
        assert torch.allclose(p, ref.detach(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(m, st["exp_avg"], rtol=1e-12, atol=0)
        assert torch.allclose(v, st["exp_avg_sq"], rtol=1e-12, atol=0)


def test_adamw_oracle_mask_is_per_64_block():
    n = 68 + 128
    p0 = torch.ones(n, dtype=torch.float64)
    z = torch.zeros(n, dtype=torch.float64)
    mask = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)  # the last block holds 4 elements
    p, _, _ = R.adamw_step64(p0, z, z, z, mask, 1.0, 1e-2, R.BETAS, 1e-8, 0.1, 1)
    exp = torch.ones(n, dtype=torch.float64)
    exp[64:128] = 1 - 1e-3
    exp[192:] = 1 - 1e-3
    assert torch.equal(p, exp)


@pytest.mark.parametrize("n", R.ADAMW_SIZES)
def test_flat_adamw_cpu_inside_gpu_bounds(n):
    """FlatAdamW(native=False) driven as the engine drives it: the oracle agrees with it (masked and
    clipped), and a correct fp32 implementation sits inside the bounds of the GPU test."""
    p0, g0 = R.adamw_inputs(n)
    mask = R.adamw_mask(n)
    opt = FlatAdamW(p0.clone(), lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD, wd_mask=mask,
                    model_bf16=torch.empty(n, dtype=torch.bfloat16))
    assert not opt.native
    R.drive_adamw(f"cpu.adamw[{n}]", opt, p0, g0, mask)
    # decay moved exactly the masked blocks: with a zero gradient nothing else moves
    opt2 = FlatAdamW(p0.clone(), lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD, wd_mask=mask)
    opt2.step()
    moved = opt2.master != p0
    assert torch.equal(moved, (mask != 0).repeat_interleave(64)[:n])


def test_flat_adamw_cpu_skip():
    n = 68
    p0, g0 = R.adamw_inputs(n)
    mask = R.adamw_mask(n)
    opt = FlatAdamW(p0.clone(), lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD, wd_mask=mask,
                    model_bf16=p0.bfloat16())
    g = g0.clone()
    g[5] = math.inf
    opt.grad.copy_(g)
    opt.set_clip(opt.local_sumsq(), 1.0)
    assert R.clip64(float(g.double().pow(2).sum()), 1.0, 1.0)[2] is True
    opt.step(use_clip=True)
    assert int(opt.skipped.item()) == 1
    assert R.bits_equal(opt.master, p0) and not opt.exp_avg.any() and not opt.exp_avg_sq.any()
    assert R.bits_equal(opt.model_bf16, p0.bfloat16())


@pytest.mark.parametrize("sumsq,max_norm,extra", R.clip_cases())
def test_clip_oracle_and_cpu_fallback(sumsq, max_norm, extra):
    opt = FlatAdamW(torch.zeros(4))
    opt.set_clip(torch.tensor([sumsq], dtype=torch.float32), max_norm, extra)
    R.check_clip("cpu.clip", opt._coef.item(), opt.grad_norm.item(), opt.skipped.item(),
                 R.f32(sumsq), max_norm, extra)


def test_clip_oracle_values():
    assert R.clip64(4.0, 1.0, 1.0) == (1.0 / (2.0 + 1e-6), 2.0, False)
    assert R.clip64(4.0, 0.0, 0.5) == (0.5, 1.0, False)
    assert R.clip64(0.25, 1.0, 1.0) == (1.0, 0.5, False)
    c, n, s = R.clip64(math.inf, 1.0, 0.125)
    assert (c, n, s) == (0.0, math.inf, True)
    c, n, s = R.clip64(math.nan, 1.0, 0.125)
    assert c == 0.125 and math.isnan(n) and s is True


@pytest.mark.parametrize("n", [4, 1020, R.SUMSQ_PASS + 4])
def test_sumsq_cpu_inside_gpu_bound(n):
    _, g = R.adamw_inputs(n, seed=7)
    opt = FlatAdamW(torch.zeros(n), grad=g)
    s64 = float(g.double().pow(2).sum())
    R.assert_within(f"cpu.sumsq[{n}]", opt.local_sumsq(), torch.tensor([s64], dtype=torch.float64), 1e-5 * s64)


# ------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("name,V,layout", R.CE_LAYOUTS, ids=[c[0] for c in R.CE_LAYOUTS])
def test_ce_oracle_matches_torch_float64(name, V, layout):
    rows, labels, kinds = R.ce_rows(V)
    x = rows.bfloat16()
    dloss = torch.randn(len(kinds), generator=torch.Generator().manual_seed(5))
    loss64, lse64, d64 = R.ce64(x, labels, R.IGNORE, dloss)
    xr = x.double().requires_grad_()
    ref = F.cross_entropy(xr, labels, ignore_index=R.IGNORE, reduction="none")
    assert torch.isfinite(ref).all(), kinds
    assert torch.allclose(loss64, ref.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(lse64, torch.logsumexp(x.double(), 1), rtol=1e-13, atol=0)
    ref.backward(dloss.double())
    assert torch.allclose(d64, xr.grad, rtol=1e-10, atol=1e-15)
    assert (loss64[labels == R.IGNORE] == 0).all() and not d64[labels == R.IGNORE].any()


@pytest.mark.parametrize("name,V,layout", R.CE_LAYOUTS, ids=[c[0] for c in R.CE_LAYOUTS])
def test_ce_cpu_fallback_inside_gpu_bounds(name, V, layout):
    rows, labels, kinds = R.ce_rows(V)
    n = len(kinds)
    st, view, _ = R.ce_place(rows, layout, "cpu")
    dloss = torch.randn(n, generator=torch.Generator().manual_seed(5))
    x = view.detach().clone().requires_grad_()
    loss = ops.cross_entropy(x, labels, ignore_index=R.IGNORE, reduction="none")
    loss.backward(dloss)
    loss64, valid = R.check_ce(f"cpu.ce[{name}].none", loss, x.grad, view, labels, dloss)
    x = view.detach().clone().requires_grad_()
    mean = ops.cross_entropy(x, labels, ignore_index=R.IGNORE, reduction="mean")
    mean.backward()
    bound, nv = R.ce_mean_bound(loss64, view, labels)
    R.assert_within(f"cpu.ce[{name}].mean", mean.reshape(1), (loss64.sum() / nv).reshape(1), bound)
    R.check_ce(f"cpu.ce[{name}].mean", loss.detach(), x.grad, view, labels, torch.full((n,), 1.0 / nv))
    assert st.intact() and R.pad_intact(st, layout, n, V)


def test_ce_rows_cover_the_edges():
    rows, labels, kinds = R.ce_rows(50257)
    assert {"spike@0", "spike@7", "spike@8", "spike@50255", "spike@50256"} <= set(kinds)
    assert {0, 50256} <= set(labels.tolist()) and (labels == R.IGNORE).sum() >= 1
    assert ((labels == R.IGNORE) | ((labels >= 0) & (labels < 50257))).all()
    # every -inf row keeps a finite logit at its label and is not ignored
    for i, k in enumerate(kinds):
        if k.startswith("neginf"):
            assert labels[i] != R.IGNORE and torch.isfinite(rows[i, labels[i]]) and torch.isinf(rows[i]).any() == (
                rows.shape[1] > 1)


# ------------------------------------------------------------------------------------ accumulate / EMA / cast
@pytest.mark.parametrize("n", R.ACCUM_SIZES)
@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_accum_expected_is_unique(n, overwrite, scale):
    """fused (double-rounded once) and unfused fp32 agree bit for bit when the scale is a power of two"""
    acc, g = R.accum_inputs(n)
    exp = R.accum_expected(acc, g, scale, overwrite)
    fused = ((0.0 if overwrite else acc.double()) + g.double() * scale).float()
    assert R.bits_equal(exp, fused)


@pytest.mark.parametrize("n", R.EMA_SIZES)
@pytest.mark.parametrize("decay", [0.999, 0.0])
def test_ema_cpu_inside_gpu_bounds(n, decay):
    shadow0, p = R.ema_inputs(n, decay)
    w = R.f32(1.0 - decay)  # what lerp_ turns its double weight into
    out = shadow0.clone().lerp_(p, 1.0 - decay)
    R.check_ema(f"cpu.ema[{n},{decay}]", out, shadow0, p, w, decay)
    # unfused fp32, written out
    out2 = shadow0 + torch.tensor(w) * (p - shadow0)
    R.check_ema(f"cpu.ema-unfused[{n},{decay}]", out2, shadow0, p, w, decay)


@pytest.mark.parametrize("n", R.CAST_SIZES)
def test_cast_inputs_and_reference(n):
    x = R.cast_inputs(n)
    y = x.to(torch.bfloat16)
    R.check_cast("cpu.cast", y, x)
    b = [v & 0xFFFF for v in y[:8].view(torch.int16).tolist()]
    assert b[:4] == [0x0000, 0x8000, 0x7F80, 0xFF80] and math.isnan(y[4].item())
    assert b[6:8] == [0x3F80, 0x3F82]  # ties to even, both parities
    if n > 8:
        assert (y[8].item(), y[9].item()) == (math.inf, -math.inf)  # largest finite fp32 rounds to inf
    trunc = (x.view(torch.int32) >> 16).to(torch.int16)
    assert not torch.equal(trunc[~torch.isnan(x)], y.view(torch.int16)[~torch.isnan(x)])  # truncation differs


def test_ulp_helpers():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 1e-45, 0.0], dtype=torch.float64)
    assert R.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]
    assert R.ulp_bf16(x[:3]).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert R.f32(0.1) == struct.unpack("f", struct.pack("f", 0.1))[0] != 0.1
    with pytest.raises(AssertionError, match="element 1"):
        R.assert_within("self-test", torch.tensor([1.0, 1.1]), torch.tensor([1.0, 1.0], dtype=torch.float64), 0.05)
    with pytest.raises(AssertionError):
        R.assert_within("self-test", torch.tensor([math.nan]), torch.tensor([1.0], dtype=torch.float64), 1.0)
    with pytest.raises(AssertionError):
        R.assert_within("self-test", torch.tensor([1.0]), torch.tensor([math.inf], dtype=torch.float64), 1.0)
    R.assert_within("self-test", torch.tensor([math.nan, -math.inf]),
                    torch.tensor([math.nan, -math.inf], dtype=torch.float64), 0.0)
    R.WORST.pop("self-test", None)


def test_guard_band():
    g = R.Guarded(8, torch.float32, "cpu")
    assert g.intact() and not g.v.any() and torch.isnan(g.buf[:R.GUARD]).all()
    g.buf[R.GUARD + 8] = 0.0
    assert not g.intact()
    for dt in (torch.bfloat16, torch.int8, torch.uint8, torch.int32):
        h = R.Guarded(4, dt, "cpu")
        assert h.intact()
        h.buf[R.GUARD - 1] = 0
        assert not h.intact()
