"""The kernels that end every optimizer step -- fused cross-entropy, fp32 gradient accumulation,
kca_sumsq, kca_clip_coef, kca_adamw / kca_adamw8bit, kca_ema, kca_cast_f32_bf16 -- per element
against the float64 oracles of tests/train_tail_ref.py (pinned on the CPU by
tests/test_train_tail_ref_cpu.py), at the sizes where each kernel takes another path: below one
vector, a ragged tail, and one vector past a full pass of the capped grid.

Every buffer a kernel writes sits between two 64-element guard bands of a sentinel bit pattern and
every test ends by checking them. Nothing here compares a norm ratio.

Worst error/bound ratio observed per check on an MI355X (1.0 is the bound; printed by every run as
"[train-tail] <name>: worst error/bound ..."):

    check                                             worst error/bound
    sumsq[n] (direct call, random data)               0.002
    adamw[n]: sumsq / norm / coef through FlatAdamW   0.010 / 0.015 / 0.012
    adamw[n]: exp_avg / exp_avg_sq / master           0.060 / 0.18 / 0.39
    adamw.shard: exp_avg / exp_avg_sq / master        0.058 / 0.15 / 0.23
    adamw.after-skip: exp_avg / exp_avg_sq / master   0.069 / 0.10 / 0.19
    adamw8bit[n]: absmax, master vs the torch twin    0 (bit-identical)
    clip: coef / norm                                 0.046 / 7e-9
    ce: loss per row / mean loss                      0.0014 / 0.0017
    ce: dlogits, reduction none / mean / one row      0.975 / 0.886 / 0.74
    ema: shadow / decay 0 equals p                    0.25 / 0 (exact)
    accumulate, cast, bf16 mirrors, skip              bit-exact checks, no bound

The dlogits ratio is that of bf16 rounding itself: round-to-nearest-even costs up to 0.996 of the
2^-8 relative term just above a power of two (tests/train_tail_ref.py, check_ce).

Two defects of csrc/kernels/cross_entropy.hip were found with these tests and are fixed there:
the forward returned lse = NaN for a row in which one thread met a -inf logit before a finite one
(rows neginf-first-half and neginf-all-but-last; NaN loss, and NaN gradients even when the row's label
is ignored), and the backward's exp(x - lse) with one fp32 lse was off by ulp(lse)/2 in the
probability, 1.12 times the dlogits bound at the label of a confident row (vector-2056, spike at the
label, lse = 20).
"""
import math

import pytest
import torch

from kubernetes_cloud_amd import ops
from kubernetes_cloud_amd.ops import _lib
from kubernetes_cloud_amd.train.optim import FlatAdamW, FlatAdamW8bit

from . import train_tail_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def G(n, dtype, init=None):
    return R.Guarded(n, dtype, DEV, init)


def _f64(x):
    return torch.tensor([x], dtype=torch.float64)


def _make_opt(cls, p0, mask, lr=R.LR):
    """A FlatAdamW(8bit) wired as TrainEngine wires it (mask, bf16 mirror, shared grad buffer), with
    every buffer the kernels write -- state and the clip scalars included -- between guard bands."""
    n = p0.numel()
    guards = {"master": G(n, F32, p0), "grad": G(n, F32), "mirror": G(n, BF16, p0.bfloat16())}
    opt = cls(guards["master"].v, lr=lr, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD,
              wd_mask=mask.to(DEV), model_bf16=guards["mirror"].v, grad=guards["grad"].v)
    assert opt.native
    state = [("_coef", 1, F32), ("_sumsq", 1, F32), ("_norm", 1, F32), ("_skip", 1, torch.int32), ("_ws", 1024, F32)]
    if cls is FlatAdamW8bit:
        nb = (n + cls.BLOCK - 1) // cls.BLOCK
        state += [("m_codes", n, torch.int8), ("v_codes", n, torch.uint8), ("m_absmax", nb, F32), ("v_absmax", nb, F32)]
    else:
        state += [("exp_avg", n, F32), ("exp_avg_sq", n, F32)]
    for name, cnt, dt in state:
        guards[name] = G(cnt, dt)
        setattr(opt, name, guards[name].v)
    opt._coef.fill_(1.0)
    return opt, guards


def _intact(guards):
    bad = [k for k, g in guards.items() if not g.intact()]
    assert not bad, f"guard band overwritten around: {bad}"


def _sumsq(g, n, ws, out):
    _lib.call("kca_sumsq", g.data_ptr(), n, ws.v.data_ptr(), out.v.data_ptr(), _lib.stream())
    return out.v.item()


# ------------------------------------------------------------------------------------ kca_sumsq
# kca_sumsq launches kca_grid(n / 4, 256, 1024) blocks: R.SUMSQ_PASS = 1024 * 256 * 4 floats fill one pass
# of the capped grid, and SUMSQ_PASS + 4 leaves exactly one float4 for the second grid-stride pass.
SUMSQ_SIZES = [4, 1020, R.SUMSQ_PASS + 4]


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_counts_every_element_once(n):
    g, ws, out = G(n, F32), G(1024, F32), G(1, F32)
    for pos in sorted({0, n - 1} | ({R.SUMSQ_PASS - 1, R.SUMSQ_PASS} if n > R.SUMSQ_PASS else set())):
        g.v[pos] = 3.0
        got = _sumsq(g.v, n, ws, out)
        assert got == 9.0, f"n={n}: a single 3.0 at index {pos} gave {got}"
        g.v[pos] = 0.0
    _intact({"g": g, "ws": ws, "out": out})


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_random_against_float64(n):
    _, x = R.adamw_inputs(n, seed=7)
    g, ws, out = G(n, F32, x), G(1024, F32), G(1, F32)
    _sumsq(g.v, n, ws, out)
    s64 = float(x.double().pow(2).sum())
    # non-negative terms, under 40 additions deep: 40 * 2^-24 = 2.4e-6
    R.assert_within(f"sumsq[{n}]", out.v, _f64(s64), 1e-5 * s64)
    _intact({"g": g, "ws": ws, "out": out})


def test_sumsq_workspace_reuse_and_nonfinite():
    n = R.SUMSQ_PASS + 4
    _, x = R.adamw_inputs(n, seed=8)
    big, ws, out = G(n, F32, x), G(1024, F32), G(1, F32)
    _sumsq(big.v, n, ws, out)  # leaves 1024 partials in the workspace
    small = G(4, F32, torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert _sumsq(small.v, 4, ws, out) == 30.0, "stale partials of the previous call were summed"
    assert _lib.call_rc("kca_sumsq", small.v.data_ptr(), 3, ws.v.data_ptr(), out.v.data_ptr(), _lib.stream()) == 1
    assert out.v.item() == 30.0
    for bad in (math.inf, -math.inf, math.nan):
        for pos in (5, R.SUMSQ_PASS + 1):
            keep = big.v[pos].item()
            big.v[pos] = bad
            assert not math.isfinite(_sumsq(big.v, n, ws, out)), (bad, pos)
            big.v[pos] = keep
    _intact({"big": big, "small": small, "ws": ws, "out": out})


# ------------------------------------------------------------------------------------ kca_clip_coef
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("extra", [1.0, 1.0 / 65536, 1.0 / 8])
def test_clip_coef(max_norm, extra):
    s, coef, norm, skip = G(1, F32), G(1, F32), G(1, F32), G(1, torch.int32)
    for sumsq, mn, ex in R.clip_cases():
        if (mn, ex) != (max_norm, extra):
            continue
        s.v.fill_(sumsq)
        coef.v.fill_(-7.0)
        norm.v.fill_(-7.0)
        skip.v.fill_(-7)
        _lib.call("kca_clip_coef", s.v.data_ptr(), mn, ex, coef.v.data_ptr(), norm.v.data_ptr(), skip.v.data_ptr(),
                  _lib.stream())
        R.check_clip(f"clip[sumsq={sumsq},max={mn},extra={ex}]", coef.v.item(), norm.v.item(), skip.v.item(),
                     R.f32(sumsq), mn, ex)
    _intact({"sumsq": s, "coef": coef, "norm": norm, "skip": skip})


# ------------------------------------------------------------------------------------ kca_adamw
# kca_adamw launches kca_grid(n / 4, 256) blocks, cap 2048: R.ADAMW_PASS = 2048 * 256 * 4 floats fill one
# pass. ADAMW_PASS + 68 crosses it and ends in a mask block of 4 elements.
@pytest.mark.parametrize("n", R.ADAMW_SIZES)
def test_adamw_as_the_engine_calls_it(n):
    p0, g0 = R.adamw_inputs(n)
    mask = R.adamw_mask(n)
    assert mask.numel() == (n + 63) // 64
    opt, guards = _make_opt(FlatAdamW, p0, mask)
    R.drive_adamw(f"adamw[{n}]", opt, p0, g0, mask)
    _intact(guards)


def test_adamw_skip_leaves_everything_bit_identical():
    n = 68
    p0, g0 = R.adamw_inputs(n)
    mask = R.adamw_mask(n)
    opt, guards = _make_opt(FlatAdamW, p0, mask)

    def engine_step(g):
        opt.grad.copy_(g)
        opt.set_clip(opt.local_sumsq(), 1.0)
        opt.step(use_clip=True)

    engine_step(g0)  # a clean step first, so the state is not all zeros
    names = ("master", "exp_avg", "exp_avg_sq", "model_bf16")
    before = {k: getattr(opt, k).clone() for k in names}
    bad = g0.clone()
    bad[5] = math.inf
    engine_step(bad)
    assert int(opt.skipped.item()) == 1
    for k in names:
        assert R.bits_equal(getattr(opt, k), before[k]), f"{k} changed in a skipped step"
    engine_step(g0 * 2)  # the following clean step updates normally
    assert int(opt.skipped.item()) == 0
    p64, m64, v64 = R.adamw_step64(before["master"].cpu(), g0 * 2, before["exp_avg"].cpu(), before["exp_avg_sq"].cpu(),
                                   mask, opt._coef.item(), R.f32(R.LR), R.BETAS, R.f32(R.EPS), R.f32(R.WD),
                                   opt.step_count)
    R.check_adamw("adamw.after-skip", 1, opt.master, opt.exp_avg, opt.exp_avg_sq, p64, m64, v64)
    assert R.bits_equal(opt.model_bf16, opt.master.cpu().to(BF16))
    _intact(guards)


def test_adamw_shard_view():
    """The ZeRO slice adamw.hip's header promises: the optimizer of master[lo:hi], lo a non-zero multiple
    of 64, with mask[lo/64:hi/64], touches nothing outside the slice."""
    N, lo, hi = 448, 128, 320
    P, Gr = R.adamw_inputs(N, seed=11)
    M = R.adamw_mask(N)  # [0, 1, 1, 0, 1, 1, 0]: the slice's [1, 0, 1] differs from the parent's first three
    master, grad, mirror = G(N, F32, P), G(N, F32, Gr), G(N, BF16, P.bfloat16())
    mask_dev = M.to(DEV)
    opt = FlatAdamW(master.v[lo:hi], lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD,
                    wd_mask=mask_dev[lo // 64:hi // 64], model_bf16=mirror.v[lo:hi], grad=grad.v[lo:hi])
    R.drive_adamw("adamw.shard", opt, P[lo:hi], Gr[lo:hi], M[lo // 64:hi // 64], ties=False)
    for name, buf, ref in (("master", master, P), ("mirror", mirror, P.bfloat16())):
        got = buf.v.cpu()
        assert R.bits_equal(got[:lo], ref[:lo]) and R.bits_equal(got[hi:], ref[hi:]), f"{name} outside [lo, hi)"
    g = grad.v.cpu()
    assert R.bits_equal(g[:lo], Gr[:lo]) and R.bits_equal(g[hi:], Gr[hi:])
    assert torch.equal(mask_dev.cpu(), M)
    _intact({"master": master, "grad": grad, "mirror": mirror})


def test_adamw_rejects_n_not_multiple_of_4():
    p0, g0 = R.adamw_inputs(8)
    bufs = {k: G(8, F32, x) for k, x in (("p", p0), ("g", g0), ("m", g0 * 0.1), ("v", g0 * g0))}
    mb = G(8, BF16, p0.bfloat16())
    before = {k: b.v.clone() for k, b in bufs.items()}
    rc = _lib.call_rc("kca_adamw", bufs["p"].v.data_ptr(), bufs["g"].v.data_ptr(), bufs["m"].v.data_ptr(),
                      bufs["v"].v.data_ptr(), mb.v.data_ptr(), 6, None, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.001,
                      None, None, _lib.stream())
    assert rc == 1
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert R.bits_equal(b.v, before[k]), k
    assert R.bits_equal(mb.v, p0.bfloat16().to(DEV))
    _intact({**bufs, "mirror": mb})


# ------------------------------------------------------------------------------------ kca_adamw8bit
@pytest.mark.parametrize("n", [4, 2048 + 4])
def test_adamw8bit_clip_skip_zero_block_and_ragged_tail(n):
    """kca_adamw8bit against the torch implementation of the same quantised math (native=False) with the
    engine's clip coefficient and skip flag. 2048 + 4 ends in a block where one thread holds four
    elements and 255 hold none; its first block has an all-zero gradient.

    The twin is reset to the kernel's state before every step, so each step is compared on its own
    (k = 1 in the master bound): one code that rounds the other way -- the codes are only held to +-1
    -- changes the next step's moment by 2/127 of itself and its update by about 1e-4, a thousand times
    the bound, without either side being wrong."""
    p0, g0 = R.adamw_inputs(n, seed=3)
    if n > 2048:
        g0[:2048] = 0.0
        g0 = R.clipped_grad(g0)
    mask = R.adamw_mask(n)
    a, guards = _make_opt(FlatAdamW8bit, p0, mask)
    b = FlatAdamW8bit(p0.clone().to(DEV), lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=R.WD, wd_mask=mask.to(DEV),
                      model_bf16=torch.empty(n, device=DEV, dtype=BF16))
    b.native = False
    state = ("master", "m_codes", "v_codes", "m_absmax", "v_absmax")
    seen = set()
    for it in range(4):
        for k in state:
            getattr(b, k).copy_(getattr(a, k))
        g = (g0 * float(1 + it)).to(DEV)
        a.grad.copy_(g)
        b.grad.copy_(g)
        a.set_clip(a.local_sumsq(), 1.0)
        b._coef.copy_(a._coef)
        b._skip.copy_(a._skip)
        coef = a._coef.item()
        assert coef < 1.0 and coef not in seen
        seen.add(coef)
        a.step(use_clip=True)
        b.step(use_clip=True)
        tag = f"adamw8bit[{n}].step{it + 1}"
        assert (a.m_codes.int() - b.m_codes.int()).abs().max() <= 1
        assert (a.v_codes.int() - b.v_codes.int()).abs().max() <= 1
        R.assert_within(f"{tag}.m_absmax", a.m_absmax, b.m_absmax.double(), 1e-6 * b.m_absmax.double().abs())
        R.assert_within(f"{tag}.v_absmax", a.v_absmax, b.v_absmax.double(), 1e-6 * b.v_absmax.double().abs())
        R.assert_within(f"{tag}.master", a.master, b.master.double(),
                        2.0 ** -22 * b.master.double().abs() + 1e-5 * R.LR)
        assert R.bits_equal(a.model_bf16, a.master.cpu().to(BF16)), f"{tag}: bf16 mirror"
        assert torch.isfinite(a.master).all() and torch.isfinite(a.m_absmax).all() and torch.isfinite(a.v_absmax).all()
        if n > 2048:  # the all-zero block: absmax and codes stay 0
            assert a.m_absmax[0].item() == 0.0 and a.v_absmax[0].item() == 0.0
            assert not a.m_codes[:2048].any() and not a.v_codes[:2048].any()
    # the planted ties (zero gradient, undecayed block 0) rounded to even in both directions
    assert a.master[1].item() == R.TIE_TO_EVEN_DOWN and a.master[2].item() == -R.TIE_TO_EVEN_UP
    assert [v & 0xFFFF for v in a.model_bf16[1:3].view(torch.int16).tolist()] == [0x3F80, 0xBF82]
    # skip: one inf in the gradient leaves codes, both absmax arrays, master and mirror bit-identical
    before = {k: getattr(a, k).clone() for k in state + ("model_bf16",)}
    g = g0.clone()
    g[n - 1] = math.inf
    a.grad.copy_(g)
    a.set_clip(a.local_sumsq(), 1.0)
    a.step(use_clip=True)
    assert int(a.skipped.item()) == 1
    for k, ref in before.items():
        assert R.bits_equal(getattr(a, k), ref), f"{k} changed in a skipped step"
    _intact(guards)


# ------------------------------------------------------------------------------------ ops.cross_entropy
def _run_ce(rows, labels, layout, reduction, inplace, dloss):
    """One forward + backward. Returns (loss, grad, logits storage after the backward as an [n, V] view,
    guarded storage). The guards and the pad columns are checked after the forward and after the
    backward."""
    n, V = rows.shape
    st, view, _ = R.ce_place(rows, layout, DEV)
    x = view.detach().requires_grad_()
    assert x.data_ptr() == view.data_ptr()
    out = ops.cross_entropy(x, labels.to(DEV), ignore_index=R.IGNORE, reduction=reduction, inplace_grad=inplace)
    torch.cuda.synchronize()
    assert st.intact() and R.pad_intact(st, layout, n, V), "forward wrote outside the logits"
    if reduction == "none":
        out.backward(dloss.to(DEV))
    else:
        out.backward()
    torch.cuda.synchronize()
    assert st.intact() and R.pad_intact(st, layout, n, V), "backward wrote outside the logits"
    return out.detach(), x.grad, view, st


@pytest.mark.parametrize("name,V,layout", R.CE_LAYOUTS, ids=[c[0] for c in R.CE_LAYOUTS])
def test_cross_entropy_per_element(name, V, layout):
    rows, labels, kinds = R.ce_rows(V)
    n = len(kinds)
    ref_logits = rows.bfloat16()
    dloss = torch.randn(n, generator=torch.Generator().manual_seed(5))
    print(f"[train-tail] ce[{name}] rows: {kinds}")
    # reduction="none" with per-row upstream gradients
    loss, grad, view, _ = _run_ce(rows, labels, layout, "none", False, dloss)
    assert R.bits_equal(view, ref_logits), "inplace_grad=False changed the logits"
    loss64, valid = R.check_ce(f"ce[{name}].none", loss, grad, ref_logits, labels, dloss)
    loss_i, grad_i, view_i, _ = _run_ce(rows, labels, layout, "none", True, dloss)
    assert R.bits_equal(loss_i, loss)
    assert R.bits_equal(grad_i, grad), "in-place backward differs from the out-of-place one"
    assert R.bits_equal(view_i, grad), "the in-place gradients are not in the logits buffer"
    # reduction="mean"
    bound, nv = R.ce_mean_bound(loss64, ref_logits, labels)
    mean, grad_m, _, _ = _run_ce(rows, labels, layout, "mean", False, None)
    R.assert_within(f"ce[{name}].mean", mean.reshape(1), (loss64.sum() / nv).reshape(1), bound)
    R.check_ce(f"ce[{name}].mean", None, grad_m, ref_logits, labels, torch.full((n,), 1.0 / nv))
    mean_i, grad_mi, view_mi, _ = _run_ce(rows, labels, layout, "mean", True, None)
    assert R.bits_equal(mean_i, mean) and R.bits_equal(grad_mi, grad_m) and R.bits_equal(view_mi, grad_m)


@pytest.mark.parametrize("name,V,layout", [R.CE_LAYOUTS[1], R.CE_LAYOUTS[4], R.CE_LAYOUTS[7]],
                         ids=["padded-50257", "vector-8", "misaligned-1000"])
def test_cross_entropy_all_labels_ignored(name, V, layout):
    rows, labels, _ = R.ce_rows(V)
    labels = torch.full_like(labels, R.IGNORE)
    for inplace in (True, False):
        mean, grad, view, _ = _run_ce(rows, labels, layout, "mean", inplace, None)
        assert mean.item() == 0.0 and math.copysign(1.0, mean.item()) == 1.0
        assert (R._bits(grad.cpu()) & 0x7FFF).eq(0).all()
        if inplace:
            assert (R._bits(view.cpu()) & 0x7FFF).eq(0).all()


@pytest.mark.parametrize("name,V,layout", [R.CE_LAYOUTS[1], R.CE_LAYOUTS[2]], ids=["padded-50257", "vector-50400"])
@pytest.mark.parametrize("row", [0, 4], ids=["neginf-first-half", "spike@0"])
def test_cross_entropy_single_row(name, V, layout, row):
    rows, labels, kinds = R.ce_rows(V)
    rows, labels = rows[row:row + 1], labels[row:row + 1]
    assert labels[0] != R.IGNORE
    dloss = torch.tensor([-0.75])
    loss, grad, _, _ = _run_ce(rows, labels, layout, "none", False, dloss)
    R.check_ce(f"ce[{name}].n1.{kinds[row]}", loss, grad, rows.bfloat16(), labels, dloss)
    loss_i, grad_i, view_i, _ = _run_ce(rows, labels, layout, "none", True, dloss)
    assert R.bits_equal(loss_i, loss) and R.bits_equal(grad_i, grad) and R.bits_equal(view_i, grad)


# ------------------------------------------------------------------------------------ accumulate / EMA / cast
# kca_accum_grad and kca_cast_f32_bf16 launch kca_grid(n / 8, 256) blocks, cap 2048: R.VEC8_PASS =
# 2048 * 256 * 8 elements fill one pass; kca_ema launches kca_grid(n / 4, 256): R.EMA_PASS = 2048 * 256 * 4.
@pytest.mark.parametrize("n", R.ACCUM_SIZES)
@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_accum_grad_bit_exact(n, overwrite, scale):
    acc0, g = R.accum_inputs(n)
    acc = G(n, F32, acc0)
    gd = g.to(DEV)
    _lib.call("kca_accum_grad", acc.v.data_ptr(), gd.data_ptr(), scale, overwrite, n, _lib.stream())
    exp = R.accum_expected(acc0, g, scale, overwrite)
    got = acc.v.cpu()
    if not R.bits_equal(got, exp):
        i = int((got.view(torch.int32) != exp.view(torch.int32)).nonzero()[0])
        raise AssertionError(f"element {i}: got {got[i].item()!r}, expected {exp[i].item()!r}")
    assert R.bits_equal(gd, g)
    _intact({"acc": acc})


@pytest.mark.parametrize("n", R.EMA_SIZES)
@pytest.mark.parametrize("decay", [0.999, 0.0])
def test_ema(n, decay):
    shadow0, p = R.ema_inputs(n, decay)
    shadow = G(n, F32, shadow0)
    pd = p.to(DEV)
    _lib.call("kca_ema", shadow.v.data_ptr(), pd.data_ptr(), decay, n, _lib.stream())
    w = 1.0 - R.f32(decay)  # the kernel's 1.f - decay, exact in fp32 for both values
    assert R.f32(w) == w
    R.check_ema(f"ema[{n},{decay}]", shadow.v, shadow0, p, w, decay)
    assert R.bits_equal(pd, p)
    _intact({"shadow": shadow})


def test_ema_and_cast_reject_ragged_sizes():
    shadow0, p = R.ema_inputs(8, 0.999)
    shadow, y = G(8, F32, shadow0), G(16, BF16)
    pd = p.to(DEV)
    assert _lib.call_rc("kca_ema", shadow.v.data_ptr(), pd.data_ptr(), 0.999, 6, _lib.stream()) == 1
    x = torch.randn(16, device=DEV)
    assert _lib.call_rc("kca_cast_f32_bf16", x.data_ptr(), y.v.data_ptr(), 12, _lib.stream()) == 1
    torch.cuda.synchronize()
    assert R.bits_equal(shadow.v, shadow0.to(DEV)) and not y.v.view(torch.int16).any()
    _intact({"shadow": shadow, "y": y})


@pytest.mark.parametrize("n", R.CAST_SIZES)
def test_cast_f32_bf16_bit_exact(n):
    x = R.cast_inputs(n)
    y = G(n, BF16)
    xd = x.to(DEV)
    _lib.call("kca_cast_f32_bf16", xd.data_ptr(), y.v.data_ptr(), n, _lib.stream())
    R.check_cast(f"cast[{n}]", y.v, x)
    _intact({"y": y})
