"""float64 oracles, input generators and per-element bounds for the kernels that end every optimizer
step: fused cross-entropy, fp32 gradient accumulation, kca_sumsq, kca_clip_coef, kca_adamw(8bit),
kca_ema and kca_cast_f32_bf16.

The oracles are written from the formulas in the kernels' header comments in plain float64 torch and
call neither FlatAdamW nor ops.cross_entropy. tests/test_train_tail_ref_cpu.py pins them against
independent implementations and shows that a correct fp32 implementation (the CPU fallback of each
op) meets every bound below; tests/test_train_tail_gpu.py applies the same generators and the same
bounds to the HIP kernels. Inputs are generated on the CPU from a seed, so both files see the same
numbers.
"""
from __future__ import annotations

import math
import struct

import torch

GUARD = 64  # elements of guard band on either side of a guarded buffer

# worst error/bound ratio seen per check name in this process (printed by every check; the table in
# test_train_tail_gpu.py's docstring is copied from it)
WORST: dict[str, float] = {}


def f32(x: float) -> float:
    """The fp32 value a ctypes c_float argument carries, as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


# ------------------------------------------------------------------------------------ guard bands
_SENTINEL = {  # by element size: NaN patterns for the float types, so a read of the band shows too
    (torch.float32, 4): (torch.int32, 0x7FC5A5A5),
    (torch.bfloat16, 2): (torch.int16, 0x7FA5),
    (torch.int8, 1): (torch.int8, -91),
    (torch.uint8, 1): (torch.uint8, 0xA5),
    (torch.int32, 4): (torch.int32, 0x5A5A5A5A),
}


def _bits(t: torch.Tensor) -> torch.Tensor:
    """Bit pattern of a contiguous tensor as a same-width integer tensor."""
    return t.contiguous().view(_SENTINEL[(t.dtype, t.element_size())][0])


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


class Guarded:
    """``n`` elements with GUARD sentinel elements before and after. ``v`` is the payload view (its
    offset, 64 elements, keeps the 16-byte alignment of the allocation for every dtype but the 1-byte
    ones, which the kernels read and write 8 bytes at a time)."""

    def __init__(self, n: int, dtype, device, init: torch.Tensor | None = None):
        idt, pat = _SENTINEL[(dtype, torch.empty(0, dtype=dtype).element_size())]
        self.n = n
        self.pat = pat
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=device)
        self.buf.view(idt).fill_(pat)
        self.v = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.v.copy_(init)
        else:
            self.v.zero_()

    def intact(self) -> bool:
        b = _bits(self.buf.cpu())
        return bool((b[:GUARD] == self.pat).all() and (b[GUARD + self.n:] == self.pat).all())


# ------------------------------------------------------------------------------------ ulp and bounds
def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |x| (float64 in, float64 out); the denormal spacing below 2^-126."""
    x = x.double().abs()
    _, e = torch.frexp(x)  # |x| = m * 2^e, m in [0.5, 1); frexp(0) has e = 0
    e = torch.where(x == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(x), (e - 24).clamp_min(-149))


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    x = x.double().abs()
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(x), (e - 8).clamp_min(-133))


def ulp_bound(x: torch.Tensor, n_ulps: float, fmt: str = "fp32") -> torch.Tensor:
    return n_ulps * (ulp32(x) if fmt == "fp32" else ulp_bf16(x))


def assert_within(name: str, actual: torch.Tensor, expected64: torch.Tensor, bound64, prefix: str = "train-tail") -> float:
    """Per element |actual - expected| <= bound. Non-finite expected values must be reproduced (NaN as
    NaN, an infinity with its sign). Prints and records the worst error/bound ratio; on failure
    reports the worst index with its values."""
    a = actual.detach().double().cpu().reshape(-1)
    e = expected64.detach().double().cpu().reshape(-1)
    b = torch.as_tensor(bound64, dtype=torch.float64).detach().cpu().expand_as(expected64.cpu()).reshape(-1)
    assert a.shape == e.shape, (name, a.shape, e.shape)
    fin = torch.isfinite(e)
    same_nonfinite = torch.where(torch.isnan(e), torch.isnan(a), a == e)
    err = torch.where(fin, (a - e).abs(), torch.zeros_like(e))
    err = torch.where(fin & ~torch.isfinite(a), torch.full_like(e, math.inf), err)
    err = torch.where(~fin & ~same_nonfinite, torch.full_like(e, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)  # bound 0 and error > 0 -> inf
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"[{prefix}] {name}: worst error/bound {worst:.3g} over {ratio.numel()} elements")
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: element {i}: got {a[i].item()!r}, expected {e[i].item()!r}, "
                             f"error {err[i].item():.3e} > bound {b[i].item():.3e} "
                             f"(ratio {worst:.3g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside)")
    return worst


# ------------------------------------------------------------------------------------ oracles
def adamw_step64(p, g, m, v, mask64, coef, lr, betas, eps, wd, step, bc=None):
    """One AdamW step of adamw.hip in float64. ``mask64``: one byte per 64-element block (None: decay
    everywhere). ``bc``: (1 - beta1^t, 1 - beta2^t) if the caller has them in another precision than
    ``betas`` (FlatAdamW computes them in double from the unrounded betas). Returns new (p, m, v)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    b1, b2 = betas
    g = g * float(coef)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = bc if bc is not None else (1.0 - b1 ** step, 1.0 - b2 ** step)
    denom = v.sqrt() / math.sqrt(bc2) + eps
    if wd != 0:
        if mask64 is None:
            dec = torch.ones_like(p, dtype=torch.bool)
        else:
            dec = (mask64.cpu() != 0).repeat_interleave(64)[:p.numel()]
        p = torch.where(dec, p * (1.0 - lr * wd), p)
    p = p - lr / bc1 * m / denom
    return p, m, v


def clip64(sumsq: float, max_norm: float, extra: float):
    """(coef, norm, skip) of clip_coef_kernel in double."""
    norm = math.sqrt(sumsq) * extra if sumsq >= 0 else math.nan  # sqrt(NaN) -> NaN
    coef = extra
    if max_norm > 0 and norm > max_norm:
        coef = extra * (max_norm / (norm + 1e-6))
    return coef, norm, (not math.isfinite(sumsq))


def ce64(logits_bf16, labels, ignore_index, dloss):
    """Per-row loss, log-sum-exp and dlogits = (softmax - onehot) * dloss[row] in float64; ignored
    rows have loss 0 and a zero gradient."""
    x = logits_bf16.detach().double().cpu()
    labels = labels.cpu()
    n, V = x.shape
    mx = x.max(dim=1, keepdim=True).values
    lse = mx.squeeze(1) + (x - mx).exp().sum(1).log()
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, safe[:, None]).squeeze(1)
    loss = torch.where(valid, lse - xl, torch.zeros_like(lse))
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    g = torch.where(valid, dloss.double().cpu(), torch.zeros(n, dtype=torch.float64))
    d = (p - onehot) * g[:, None]
    d[~valid] = 0.0
    return loss, lse, d


def ema64(shadow, p, w: float):
    """shadow + w * (p - shadow) with w = 1 - decay as the caller's arithmetic has it."""
    return shadow.double() + w * (p.double() - shadow.double())


# ------------------------------------------------------------------------------------ AdamW inputs
# Grid caps, from kca_grid(work_items, 256 threads, cap) in csrc/kernels: one thread takes one 16-byte
# vector per pass, so one pass of the capped grid is cap * 256 * (elements per vector) elements.
#   kca_sumsq          kca_grid(n / 4, 256, 1024)         -> 1024 * 256 * 4 floats
#   kca_adamw, kca_ema kca_grid(n / 4, 256) (cap 2048)    -> 2048 * 256 * 4 floats
#   kca_accum_grad, kca_cast_f32_bf16  kca_grid(n / 8, 256) (cap 2048) -> 2048 * 256 * 8 elements
SUMSQ_PASS = 1024 * 256 * 4
ADAMW_PASS = 2048 * 256 * 4
EMA_PASS = 2048 * 256 * 4
VEC8_PASS = 2048 * 256 * 8

ADAMW_SIZES = [4, 68, ADAMW_PASS + 68]
LR, WD, EPS = 1e-2, 0.1, 1e-8
# Betas that fp32 holds exactly, as are 1 - beta: the kernel takes them as fp32 and forms 1.f - beta,
# the torch fallback rounds beta and 1 - beta to fp32 separately, and for 0.999 those two differ by
# 1.3e-5 relative, thirteen times the bound on exp_avg_sq. With dyadic betas every implementation and
# the oracle use the same four numbers and the bounds measure the arithmetic alone.
BETAS = (0.875, 1.0 - 2.0 ** -10)
# both parities of an exact fp32 -> bf16 rounding tie, inside |p| in [0.5, 2]
TIE_TO_EVEN_DOWN = struct.unpack("f", struct.pack("I", 0x3F808000))[0]  # -> 0x3F80
TIE_TO_EVEN_UP = struct.unpack("f", struct.pack("I", 0x3F818000))[0]    # -> 0x3F82


def adamw_mask(n: int) -> torch.Tensor:
    return (torch.arange((n + 63) // 64) % 3 != 0).to(torch.uint8)


def adamw_inputs(n: int, seed: int = 0):
    """(p0, g0): |p| in [0.5, 2] with random sign, g ~ N(0, 1). Elements 1 and 2 lie in block 0, which
    the mask never decays; their gradient is zero, so their moments and update stay zero and the
    masters planted there remain exactly on a bf16 rounding tie through every step."""
    gen = torch.Generator().manual_seed(seed)
    p = (0.5 + 1.5 * torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    g = torch.randn(n, generator=gen)
    p[1], p[2] = TIE_TO_EVEN_DOWN, -TIE_TO_EVEN_UP
    g[1] = g[2] = 0.0
    return p, clipped_grad(g)


def clipped_grad(g):
    """g scaled up, if need be, to a norm of at least 3, so that max_norm = 1 clips it in every step."""
    return g * max(1.0, 3.0 / float(g.norm()))


def check_adamw(tag, k, p, m, v, p64, m64, v64):
    """The per-element bounds after k steps (issue text): two roundings of p per step cost
    2 * 2^-24 |p|, the update term is at most about 3 lr and is a handful of fp32 operations."""
    assert_within(f"{tag}.exp_avg", m, m64, k * 1e-6 * m64.abs())
    assert_within(f"{tag}.exp_avg_sq", v, v64, k * 1e-6 * v64.abs() + 1e-30)
    assert_within(f"{tag}.master", p, p64, k * (2.0 ** -22 * p64.abs() + 1e-5 * LR))


def drive_adamw(tag, opt, p0, g0, mask, steps=4, max_norm=1.0, ties=True):
    """Run ``opt`` (a FlatAdamW whose buffers already hold p0, on any device) the way TrainEngine does:
    local_sumsq, set_clip, step(use_clip=True), with the gradient scaled by (1 + step) so that the clip
    coefficient is below 1 and different in every step. After every step: sumsq and the coefficient
    against float64, then exp_avg, exp_avg_sq and master per element against the float64 trajectory
    fed the same fp32 gradient and the coefficient the optimizer used, and the bf16 mirror bit for
    bit."""
    p64, m64, v64 = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    seen = set()
    for s in range(steps):
        g = g0 * float(1 + s)
        opt.grad.copy_(g)
        ss = opt.local_sumsq()
        opt.set_clip(ss, max_norm)
        opt.step(use_clip=True)
        ss64 = float(g.double().pow(2).sum())
        assert_within(f"{tag}.sumsq", ss, torch.tensor([ss64], dtype=torch.float64), 1e-5 * ss64)
        coef = float(opt._coef.item())
        c64, n64, _ = clip64(ss64, max_norm, 1.0)
        # sumsq is within 1e-5, its square root within 5e-6; kca_clip_coef adds 1e-6
        assert_within(f"{tag}.coef", opt._coef, torch.tensor([c64], dtype=torch.float64), 6e-6 * c64)
        assert_within(f"{tag}.norm", opt.grad_norm, torch.tensor([n64], dtype=torch.float64), 6e-6 * n64)
        assert coef < 1.0 and coef not in seen, (tag, s, coef)
        seen.add(coef)
        assert int(opt.skipped.item()) == 0
        p64, m64, v64 = adamw_step64(p64, g, m64, v64, mask, coef, f32(LR), BETAS, f32(EPS), f32(WD), s + 1)
        check_adamw(f"{tag}.step{s + 1}", s + 1, opt.master, opt.exp_avg, opt.exp_avg_sq, p64, m64, v64)
        assert bits_equal(opt.model_bf16, opt.master.cpu().to(torch.bfloat16)), f"{tag}: bf16 mirror, step {s + 1}"
    # the planted ties never moved, and rounded to even in both directions
    if ties:
        assert opt.master[1].item() == TIE_TO_EVEN_DOWN and opt.master[2].item() == -TIE_TO_EVEN_UP
        mb = _bits(opt.model_bf16[1:3].cpu()).tolist()
        assert [b & 0xFFFF for b in mb] == [0x3F80, 0xBF82], [hex(b & 0xFFFF) for b in mb]
    return p64, m64, v64


# ------------------------------------------------------------------------------------ clip cases
def clip_cases():
    """(sumsq, max_norm, extra_scale). With extra_scale 1 and max_norm 1 the norms are 0, 0.5,
    1 - 2^-24, 1, 1 + 2^-23, 3 and 1e5: below, within one fp32 ulp on either side of, exactly at, and
    above max_norm. The near cases are squares chosen so that fp32 and double take the same side of
    `norm > max_norm` (sqrt(1 - 2^-23) < 1 and sqrt(1 + 2^-22) > 1 in both); at the threshold itself
    the coefficient jumps by 1e-6, so a case on which the two precisions disagree would test the
    rounding of sqrtf, not the kernel."""
    sums = [0.0, 0.25, 1.0 - 2.0 ** -23, 1.0, 1.0 + 2.0 ** -22, 9.0, 1e10, math.inf, math.nan]
    return [(s, mn, ex) for s in sums for mn in (0.0, 1.0) for ex in (1.0, 1.0 / 65536, 1.0 / 8)]


def check_clip(tag, coef, norm, skip, sumsq, max_norm, extra):
    c64, n64, s64 = clip64(sumsq, max_norm, extra)
    # five fp32 operations: at most 5 * 2^-24 relative
    assert_within(f"{tag}.coef", torch.tensor([coef]), torch.tensor([c64], dtype=torch.float64), 1e-6 * abs(c64))
    assert_within(f"{tag}.norm", torch.tensor([norm]), torch.tensor([n64], dtype=torch.float64), 1e-6 * abs(n64))
    assert int(skip) == int(s64), (tag, sumsq, skip)
    if sumsq == 0.0:
        assert struct.pack("f", coef) == struct.pack("f", extra), (tag, coef, extra)


# ------------------------------------------------------------------------------------ cross-entropy
IGNORE = -100
NEG_INF = -math.inf
# (name, V, layout)
CE_LAYOUTS = [
    ("scalar-50257", 50257, "contig"),      # ld % 8 != 0 -> scalar kernels
    ("padded-50257", 50257, "padded"),      # columns [:V] of [n, 50264]: vector kernels + 1-element tail
    ("vector-50400", 50400, "contig"),      # GPT-J: vector, no tail
    ("vector-2056", 2056, "contig"),        # 257 vectors: a second trip for thread 0 only
    ("vector-8", 8, "contig"),              # one vector, 255 idle threads
    ("scalar-7", 7, "contig"),
    ("single-class", 1, "contig"),
    ("misaligned-1000", 1000, "offset1"),   # ld % 8 == 0 but the base is 2 bytes past 16-byte alignment
]


def ce_rows(V: int, seed: int = 0):
    """(logits fp32 [n, V] holding bf16-representable values after .bfloat16(), labels [n], kinds)."""
    gen = torch.Generator().manual_seed(seed + V)
    rows, kinds, labels = [], [], []
    cyc = [0, V - 1, 8 * (V >> 3) if 8 * (V >> 3) < V else V // 2]  # first, last, first tail element

    def add(kind, row, label=None):
        labels.append(cyc[len(rows) % 3] if label is None else label)
        rows.append(row)
        kinds.append(kind)

    idx = torch.arange(V)
    # -inf rows first, so the every-seventh ignore below never lands on one; labels on finite logits
    r = torch.randn(V, generator=gen)
    r[:V // 2] = NEG_INF
    add("neginf-first-half", r, V - 1)
    r = torch.randn(V, generator=gen)
    r[(idx // 8) % 2 == 1] = NEG_INF  # vector 0 stays finite, so no row is all -inf
    add("neginf-odd-vectors", r, 0)
    r = torch.randn(V, generator=gen)
    r[:V - 1] = NEG_INF
    add("neginf-all-but-last", r, V - 1)
    add("randn3", 3 * torch.randn(V, generator=gen))
    for pos in sorted({0, 7, 8, 8 * (V >> 3) - 1, 8 * (V >> 3), V - 1}):
        if 0 <= pos < V:
            r = torch.randn(V, generator=gen)
            r[pos] = 20.0
            add(f"spike@{pos}", r)
    ramp = torch.linspace(-30, 30, V) if V > 1 else torch.zeros(1)
    add("ramp-up", ramp.clone())
    add("ramp-down", ramp.flip(0).clone())
    r = torch.full((V,), -3e4)
    r[(V * 2) // 3] = 3e4
    add("one-hot-3e4", r)
    add("constant", torch.full((V,), 1.5))
    labels = torch.tensor(labels, dtype=torch.int64)
    labels[3::7] = IGNORE
    assert 9 <= len(rows) <= 16
    return torch.stack(rows), labels, kinds


def ce_place(rows_f32: torch.Tensor, layout: str, device):
    """Lay the rows out as the case asks, inside a guarded bf16 storage. Returns (guarded storage,
    logits view [n, V], pad view or None)."""
    n, V = rows_f32.shape
    x = rows_f32.bfloat16()
    if layout == "contig":
        st = Guarded(n * V, torch.bfloat16, device)
        view = st.v.view(n, V)
        pad = None
    elif layout == "padded":
        ld = (V + 7) // 8 * 8 if V % 8 else V + 8
        st = Guarded(n * ld, torch.bfloat16, device)
        st.v.view(torch.int16).fill_(st.pat)
        full = st.v.view(n, ld)
        view, pad = full[:, :V], full[:, V:]
    elif layout == "offset1":
        st = Guarded(n * V + 8, torch.bfloat16, device)
        st.v.view(torch.int16).fill_(st.pat)
        view = st.v[1:1 + n * V].view(n, V)
        pad = torch.cat([st.v[:1], st.v[1 + n * V:]])
    else:
        raise ValueError(layout)
    view.copy_(x)
    return st, view, pad


def pad_intact(st: Guarded, layout: str, n: int, V: int) -> bool:
    b = _bits(st.v.cpu())
    if layout == "padded":
        ld = b.numel() // n
        return bool((b.view(n, ld)[:, V:] == st.pat).all())
    if layout == "offset1":
        return bool((b[:1] == st.pat).all() and (b[1 + n * V:] == st.pat).all())
    return True


def check_ce(tag, loss, grad, logits_bf16, labels, dloss):
    """Per-row loss and per-element gradient bounds of the issue against ce64."""
    loss64, lse64, d64 = ce64(logits_bf16, labels, IGNORE, dloss)
    x = logits_bf16.detach().double().cpu()
    lab = labels.cpu()
    n, V = x.shape
    valid = lab != IGNORE
    xl = x.gather(1, torch.where(valid, lab, torch.zeros_like(lab))[:, None]).squeeze(1)
    assert torch.isfinite(loss64).all()
    # the row sum is 256 threads of at most 200 fp32 additions of positive terms: 200 * 2^-24 = 1.2e-5,
    # plus __logf
    lb = 5e-5 * torch.maximum(torch.ones_like(lse64), torch.maximum(lse64.abs(), xl.abs()))
    lb = torch.where(valid, lb, torch.zeros_like(lb))  # ignored rows: exactly 0
    if loss is not None:
        assert_within(f"{tag}.loss", loss, loss64, lb)
    if grad is None:
        return loss64, valid
    dl = dloss.double().cpu().abs()
    # bf16 keeps 8 significant bits: round-to-nearest-even alone costs up to 2^-8 / (1 + 2^-8) of the value
    # (just above a power of two), 0.996 of the relative term, so a correct kernel is seen close to this
    # bound; the fp32 error of exp and of the row sum (about 1e-5 relative) has the rest and the
    # absolute term
    gb =2.0 ** -8 * d64.abs() + 1e-6 * dl[:, None]
    gb[~valid] = 0.0
    assert_within(f"{tag}.dlogits", grad, d64, gb)
    g = grad.detach().cpu()
    assert (_bits(g[~valid]) & 0x7FFF).eq(0).all(), f"{tag}: ignored rows must be zero bit patterns"
    g64 = g.double()
    rs = g64.sum(1).abs()
    rb = V * 2.0 ** -9 * g64.abs().max(1).values
    assert (rs <= rb).all(), f"{tag}: row sums {rs.tolist()} exceed {rb.tolist()}"
    return loss64, valid


def ce_mean_bound(loss64, logits_bf16, labels):
    """|mean - mean64| for reduction='mean': the per-row bounds averaged, plus the fp32 sum of at most
    16 rows and one division (17 * 2^-24 of sum |loss|, taken as 2^-19)."""
    x = logits_bf16.detach().double().cpu()
    lab = labels.cpu()
    valid = lab != IGNORE
    nv = max(int(valid.sum()), 1)
    lse = torch.logsumexp(x, 1)
    xl = x.gather(1, torch.where(valid, lab, torch.zeros_like(lab))[:, None]).squeeze(1)
    lb = 5e-5 * torch.maximum(torch.ones_like(lse), torch.maximum(lse.abs(), xl.abs()))
    return float((lb[valid].sum() + 2.0 ** -19 * loss64.abs().sum()) / nv), nv


# ------------------------------------------------------------------------------------ accumulate / EMA / cast
ACCUM_SIZES = [3, 8, 11, VEC8_PASS + 11]
EMA_SIZES = [4, EMA_PASS + 4]
CAST_SIZES = [8, VEC8_PASS + 8]


def accum_inputs(n: int, seed: int = 0):
    gen = torch.Generator().manual_seed(seed + 1)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen).bfloat16()


def accum_expected(acc, g_bf16, scale, overwrite):
    """With a power-of-two scale g * scale is exact, so a fused and an unfused multiply-add agree and
    the fp32 result is unique."""
    base = torch.zeros_like(acc) if overwrite else acc
    return base + g_bf16.float() * scale


def ema_inputs(n: int, decay: float, seed: int = 0):
    """decay 0.999: shadow, p ~ N(0, 1). decay 0: both in [1, 2) with a common sign per element, so
    p - shadow is exact (Sterbenz) and shadow + 1 * (p - shadow) is p itself up to the one rounding the
    issue allows; for unrelated magnitudes (p = 1e-4, shadow = 2) a correct fp32 kernel is off by
    ulp(shadow)/2, thousands of ulps of p."""
    gen = torch.Generator().manual_seed(seed + 2)
    if decay == 0:
        sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
        return sign * (1 + torch.rand(n, generator=gen)), sign * (1 + torch.rand(n, generator=gen))
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen)


def check_ema(tag, out, shadow0, p, w, decay):
    e64 = ema64(shadow0, p, w)
    d = (p.double() - shadow0.double()).abs()
    assert_within(f"{tag}.shadow", out, e64, 2 * ulp32(e64) + 2.0 ** -23 * d)
    if decay == 0:
        assert_within(f"{tag}.equals-p", out, p.double(), ulp32(p.double()))


def _f(bits: int) -> float:
    return struct.unpack("f", struct.pack("I", bits))[0]


CAST_SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 1e-40, TIE_TO_EVEN_DOWN, TIE_TO_EVEN_UP,
                 # the rest only where there is room (n > 8)
                 _f(0x7F7FFFFF), -_f(0x7F7FFFFF), -1e-40, _f(0x00000001), -TIE_TO_EVEN_DOWN, -TIE_TO_EVEN_UP,
                 _f(0x3F807FFF), _f(0x3F808001), _f(0x7F7F8000), _f(0x007FFFFF)]


def cast_inputs(n: int, seed: int = 0):
    """Specials at the head (and, when there is room, again at the very end: the second grid-stride
    pass), random numbers with random exponents between."""
    gen = torch.Generator().manual_seed(seed + 3)
    x = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-20, 20, (n,), generator=gen).float())
    sp = torch.tensor(CAST_SPECIALS[:min(n, len(CAST_SPECIALS))])
    x[:sp.numel()] = sp
    if n >= 2 * sp.numel():
        x[-sp.numel():] = sp
    return x


def check_cast(tag, y_bf16, x_f32):
    """Bit-identical to torch's round-to-nearest-even cast; a NaN must stay a NaN (payload free)."""
    ref = x_f32.cpu().to(torch.bfloat16)
    y = y_bf16.cpu()
    nan = torch.isnan(ref)
    assert torch.isnan(y[nan]).all(), f"{tag}: NaN did not stay NaN"
    rb, yb = _bits(ref), _bits(y)
    bad = (rb != yb) & ~nan
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{tag}: element {i}: {x_f32.cpu()[i].item()!r} -> bits {int(yb[i]) & 0xFFFF:#06x}, "
                             f"expected {int(rb[i]) & 0xFFFF:#06x} ({int(bad.sum())} elements differ)")
