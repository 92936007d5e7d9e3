"""float64 oracles, per-element bounds and seeded inputs for the normalisation kernels:
csrc/kernels/layernorm.hip, groupnorm.hip (NCHW) and groupnorm_nhwc.hip (channels-last, with the
fused per-(n, c) add and the concat / phase-layout forms).

Every formula below is written once, generic over the dtype it is evaluated in. In float64 it is the
oracle (tests/test_norm_ref_cpu.py pins it against F.layer_norm / F.group_norm / F.silu with autograd);
in float32 it is the "plain fp32 evaluation of the same formula on the same inputs" from which the
fp32 part of every bound is taken. The backward formulas are written out, not taken from autograd.

Bounds (no constant in them is fitted to a kernel):

  bf16 outputs (h aside)   |out - ref| <= 2^-8 |ref| + T
      Rounding the exact result to bf16 (8 significant bits, round to nearest even) costs at most half
      a unit in the last place, 2^-9 of the next power of two above |ref|, which is at most
      2^-8 |ref| and reaches 0.996 of it just above a power of two (the form check_ce uses).
  fp32 outputs             |out - ref| <= T
      mean, rstd, and dgamma / dbeta when the kernel writes them as fp32.
  T, per element outputs   4 x the largest deviation of the fp32 evaluation from the oracle over the
      same row (LayerNorm) or (n, g) group (GroupNorm) -- four, because the summation orders differ
      (tests/test_decode_fp16_gpu.py).
  T, mean and rstd         one number per row or group, so "the largest deviation over the same row"
      is a single sample of an fp32 evaluation's error, not a bound on another's: against four times
      it torch.native_layer_norm, a correct fp32 implementation, is off by 2.9 bounds on the mean of a
      9 x 2056 randn case (1.4e-8 against 5e-9; tests/test_norm_ref_cpu.py runs it under the bounds
      used instead). The statistics are
      reductions and get the reduced form instead, with k_s the longest addition chain of the row or
      group sum (ln_stat_chain / nchw_stat_chain / nhwc_stat_chain):
        mean  T = k_s 2^-24 sum |x| / L          the sum cancels; its error is relative to sum |x|
        rstd  T = (k_s / 2 + 3) 2^-24 rstd        the variance is a sum of squares about the mean (no
              cancellation: the two-pass, shifted and Welford forms the kernels use all promise this),
              relative error k_s 2^-24, halved by the square root, plus the addition of eps, rsqrtf
              (1 ulp = 2^-23) and the final rounding.
      A divisor off by one moves rstd by 1 / (2d): 3e-5 at d = 16384 against 2.5e-6.
  Carried statistics       y and dx are functions of mean and rstd, one sample of whose error shifts a
      whole row or group at once (at a mean of 50 standard deviations it is the whole fp32 error of
      y near 0: F.layer_norm in fp32 is 1.45 x 4 deviations of the evaluation here on a 67 x 520
      case), so the two bounds above are carried through to first order (stat_terms_y,
      stat_terms_dx) and added to T; the backward kernels are handed the forward's mean and rstd.
  T, reduced outputs       dgamma, dbeta, dw, db are sums over rows or pixels:
      T = k 2^-24 sum |terms|, k = the longest chain of additions a partial sum goes through in the
      kernel (read from the code; ln_chain / nchw_chain / nhwc_chain below state it) plus K_TERM = 16
      for the roundings inside one term. A dgamma term is dy (h - mean) rstd: its fp32 error is
      relative to |h| + |mean| (what is subtracted), not to the difference, so the terms summed are
      |dy| (|h| + |mean|) rstd; mean and rstd carry their own few roundings, then come the subtraction,
      two products and, with SiLU, the derivative through __expf (about |z| 2^-23 relative).

The fp32 evaluation of the GroupNorm forward and of the channels-last backward uses the folded form
the kernels document (y = x * scale + shift with shift = beta - mean * scale; dx = sc * dz + B * x + Cc):
at a group mean of 50 standard deviations the two products cancel and that form is what fp32 costs.

Inputs are generated on the CPU from a seed and hold bf16-representable values.
"""
from __future__ import annotations

import math

import torch

from .train_tail_ref import GUARD, WORST, Guarded, assert_within, bits_equal, f32, ulp32, ulp_bf16  # noqa: F401

BF16 = torch.bfloat16
F64 = torch.float64
F32 = torch.float32
EPS = f32(1e-5)  # what a ctypes c_float carries
K_TERM = 16
BIG = 8.0  # planted magnitude
TINY = 2.0 ** -6  # scale of everything that is not planted


# ------------------------------------------------------------------------------------ checking
def within(name: str, actual, expected64, bound64, check: bool = True) -> float:
    """assert_within under the "norm" prefix; with check=False only the worst error/bound ratio is
    returned (the sensitivity tests want to see it exceed 1)."""
    if check:
        return assert_within(name, actual, expected64, bound64, prefix="norm")
    a = actual.detach().double().cpu().reshape(-1)
    e = expected64.detach().double().cpu().reshape(-1)
    b = torch.as_tensor(bound64, dtype=F64).expand_as(expected64).reshape(-1)
    fin = torch.isfinite(e)
    err = torch.where(fin, (a - e).abs(), torch.zeros_like(e))
    err = torch.where(fin & ~torch.isfinite(a), torch.full_like(e, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(ratio.max()) if ratio.numel() else 0.0


def _dev(e32, ref64, dims):
    """Largest |fp32 evaluation - oracle| over ``dims``, kept for broadcasting."""
    return (e32.double() - ref64).abs().amax(dims, keepdim=True)


def bound_bf16(ref64, e32, dims):
    return 2.0 ** -8 * ref64.abs() + 4.0 * _dev(e32, ref64, dims)


def bound_mean(absmean64, k: int):
    """absmean64: sum |x| / L per row or group."""
    return k * 2.0 ** -24 * absmean64


def bound_rstd(rstd64, k: int):
    return (k / 2 + 3) * 2.0 ** -24 * rstd64


def bound_reduced(ref64, terms64, k: int, bf16_out: bool):
    t = k * 2.0 ** -24 * terms64
    return 2.0 ** -8 * ref64.abs() + t if bf16_out else t


# ------------------------------------------------------------------------------------ LayerNorm
def ln_h(x, res):
    """(exact float64 sum, the bf16 h the kernel claims: fp32 adds left to right, one rounding)."""
    h64, h32 = x.double(), x.float()
    for r in res:
        h64 = h64 + r.double()
        h32 = h32 + r.float()
    return h64, h32.to(BF16)


def ln_fwd(h, gamma, beta, eps=EPS, dt=F64):
    """mean, rstd, y of LayerNorm over the last dim of the bf16 ``h`` (the rounded residual sum: what
    the kernel normalises and the backward re-reads)."""
    hb = h.to(dt)
    d = hb.shape[-1]
    mean = hb.sum(-1) / d
    c = hb - mean[:, None]
    var = (c * c).sum(-1) / d
    rstd = (var + eps).rsqrt() if dt == F32 else 1.0 / (var + eps).sqrt()
    zc = c * rstd[:, None] * gamma.to(dt)
    y = zc + beta.to(dt) if beta is not None else zc
    return {"mean": mean, "rstd": rstd, "y": y, "stat": stat_terms_y(rstd[:, None], gamma.to(dt), zc)}


def ln_bwd(dy, h, gamma, dres=None, eps=EPS, dt=F64):
    """dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) (+ dres); dgamma = sum_rows dy xhat;
    dbeta = sum_rows dy; and the sums of |terms| the reduced bounds need."""
    hb, g, dyv = h.to(dt), gamma.to(dt), dy.to(dt)
    d = hb.shape[-1]
    mean = hb.sum(-1, keepdim=True) / d
    c = hb - mean
    var = (c * c).sum(-1, keepdim=True) / d
    rstd = (var + eps).rsqrt() if dt == F32 else 1.0 / (var + eps).sqrt()
    xh = c * rstd
    gy = dyv * g
    m1 = gy.sum(-1, keepdim=True) / d
    m2 = (gy * xh).sum(-1, keepdim=True) / d
    dx = rstd * (gy - m1 - xh * m2)
    if dres is not None:
        dx = dx + dres.to(dt)
    return {"dx": dx, "dgamma": (dyv * xh).sum(0), "dbeta": dyv.sum(0),
            "t_dgamma": (dyv.abs() * (hb.abs() + mean.abs()) * rstd).sum(0), "t_dbeta": dyv.abs().sum(0),
            "stat": stat_terms_dx(rstd, xh, m1, m2, dx - dres.to(dt) if dres is not None else dx),
            "rstd": rstd, "xh": xh}


def stat_terms_y(rstd, gw, zc, silu_on=False):
    """How an error of the statistics moves y = act((x - mean) rstd gamma + beta): (per unit of mean
    error, per unit of relative rstd error). zc = z - beta; |silu'| <= 1.1."""
    a = 1.1 if silu_on else 1.0
    return a * rstd * gw.abs(), a * zc.abs()


def stat_terms_dx(rstd, xh, m1, m2, dx0, extra=None):
    """The same for dx = rstd (gy - m1 - xhat m2), to first order. A mean error e shifts xhat by
    -rstd e and m2 by -m1 rstd e: dx moves by rstd^2 e (m2 + xhat m1). A relative rstd error r
    scales xhat and m2: dx moves by r (dx - 2 rstd xhat m2). ``extra``: (per mean, per rstd) the
    SiLU derivative adds (GroupNorm)."""
    pm = rstd * rstd * (m2.abs() + (xh * m1).abs())
    pr = dx0.abs() + 2 * rstd * (xh * m2).abs()
    if extra is not None:
        pm, pr = pm + extra[0], pr + extra[1]
    return pm, pr


def bound_elem(ref64, e32, dims, stat, bm, br_rel):
    """bf16 per-element bound: rounding, 4 x the fp32 evaluation's deviation, and the statistics'
    own bounds carried through ``stat`` = (per unit mean error, per unit relative rstd error)."""
    return bound_bf16(ref64, e32, dims) + stat[0] * bm + stat[1] * br_rel


def ln_parts(rows: int) -> int:
    return rows if 0 < rows < 1024 else (1 if rows <= 0 else 1024)  # kca_layernorm_bwd_parts


def ln_chain(rows: int, d: int, narrow: bool) -> int:
    """Longest addition chain of a dgamma / dbeta partial in layernorm.hip: a register accumulator
    over the rows one workgroup (block kernel) or one wave (narrow kernel: 4 waves, then a 4-way sum
    through LDS) takes, then col_reduce64 (d % 64 == 0: ceil(parts / 16) strided additions and a
    16-way fold) or col_reduce (all parts in sequence)."""
    parts = ln_parts(rows)
    k = -(-rows // (parts * 4)) + 3 if narrow else -(-rows // parts)
    k += -(-parts // 16) + 15 if d % 64 == 0 else parts
    return k + K_TERM


def ln_stat_chain(d: int) -> int:
    """ln_fwd_kernel's row sum: NV x 8 additions in a thread, 6 wave shuffles, up to 4 waves, the
    division."""
    return ln_nv(d) * 8 + 6 + 4 + 1


def ln_narrow(d: int, knob: bool = True) -> bool:
    return d <= 1024 and knob


def ln_nv(d: int) -> int:
    return max(1, (d // 8 + 255) // 256)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _params(n, g, beta=True):
    gamma = (1 + 0.1 * torch.randn(n, generator=g)).to(BF16)
    b = (0.1 * torch.randn(n, generator=g)).to(BF16) if beta else None
    return gamma, b


def ln_marks(d: int):
    """First and last element of the row and both sides of every boundary the kernels have: the first
    and last 16-byte vector, a wave's 64 vectors (512 elements: the narrow kernel's second pass) and a
    workgroup's 256 vectors (2048 elements: the NV loop)."""
    m = {0, 7, 8, d - 9, d - 8, d - 1}
    for step in (512, 2048):
        for e in range(step, d, step):
            m |= {e - 1, e}
    return sorted(i for i in m if 0 <= i < d)


def ln_cases(rows: int, d: int, nres: int = 0, beta: bool = True, dres: bool = False, seed: int = 0):
    """{name: case}; a case holds x, res (list), gamma, beta, dy, dres -- bf16 on the CPU."""
    g = _gen(seed * 1000003 + rows * 131 + d)
    gamma, b = _params(d, g, beta)

    def mk(x, dy, scale=1.0):
        res = [(scale * torch.randn(rows, d, generator=g)).to(BF16) for _ in range(nres)]
        dr = torch.randn(rows, d, generator=g).to(BF16) if dres else None
        return {"x": x.to(BF16), "res": res, "gamma": gamma, "beta": b, "dy": dy.to(BF16), "dres": dr,
                "rows": rows, "d": d}

    out = {"uniform": mk(torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g))}
    # a row mean of about 50 standard deviations
    out["offset"] = mk(50.0 + torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g))
    # variance 0: 1.5 sums exactly in fp32 in any order up to d = 16384, so mean is exact, rstd is
    # eps^-1/2 and y is beta; the residuals are zero
    c = mk(torch.full((rows, d), 1.5), torch.randn(rows, d, generator=g), scale=0.0)
    out["constant"] = c
    marks = torch.tensor(ln_marks(d))
    sign = torch.where(torch.arange(marks.numel()) % 2 == 0, BIG, -BIG)
    x = TINY * torch.randn(rows, d, generator=g)
    dy = TINY * torch.randn(rows, d, generator=g)
    x[:, marks] = sign
    dy[:, marks] = sign.flip(0) if marks.numel() > 1 else sign
    out["planted"] = mk(x, dy, scale=TINY)
    return out


def poison_rows(t: torch.Tensor, row: int):
    """A copy of ``t`` ([rows, d] or [N, G, L]) whose ``row`` holds NaN, +inf and -inf."""
    t = t.clone()
    flat = t[row].reshape(-1)
    flat[0] = math.nan
    flat[flat.numel() // 2] = math.inf
    flat[-1] = -math.inf
    t[row] = flat.view_as(t[row])
    return t


def check_ln_fwd(tag, c, got, check=True):
    """got: h (None without residuals), y, mean, rstd. h within one bf16 ulp of the exact sum and with
    exactly the rounding the kernel claims; y, mean, rstd against the oracle fed the h that was
    stored."""
    w = {}
    if c["res"]:
        h64, claim = ln_h(c["x"], c["res"])
        w["h"] = within(f"{tag}.h", got["h"], h64, ulp_bf16(h64), check)
        if check:
            assert bits_equal(got["h"].cpu().reshape(claim.shape), claim), f"{tag}: h is not the fp32 sum rounded once"
        h = got["h"].cpu().reshape(claim.shape)
    else:
        h = c["x"]
    o, e = ln_fwd(h, c["gamma"], c["beta"]), ln_fwd(h, c["gamma"], c["beta"], dt=F32)
    ks = ln_stat_chain(c["d"])
    bm, br = bound_mean(h.double().abs().mean(-1), ks), bound_rstd(o["rstd"], ks)
    if got.get("mean") is not None:  # (the autograd ops do not hand them out)
        w["mean"] = within(f"{tag}.mean", got["mean"], o["mean"], bm, check)
        w["rstd"] = within(f"{tag}.rstd", got["rstd"], o["rstd"], br, check)
    by = bound_elem(o["y"], e["y"], -1, o["stat"], bm[:, None], (br / o["rstd"])[:, None])
    w["y"] = within(f"{tag}.y", got["y"], o["y"], by, check)
    return w


def check_ln_bwd(tag, c, h, got, narrow, params_fp32, check=True):
    """got: dx, dgamma, dbeta (None without beta)."""
    o = ln_bwd(c["dy"], h, c["gamma"], c["dres"])
    e = ln_bwd(c["dy"], h, c["gamma"], c["dres"], dt=F32)
    k = ln_chain(c["rows"], c["d"], narrow)
    ks = ln_stat_chain(c["d"])  # the backward is handed the forward's fp32 mean and rstd
    bm, rr = bound_mean(h.double().abs().mean(-1, keepdim=True), ks), bound_rstd(1.0, ks)
    w = {"dx": within(f"{tag}.dx", got["dx"], o["dx"], bound_elem(o["dx"], e["dx"], -1, o["stat"], bm, rr), check)}
    sfx = "32" if params_fp32 else ""
    sg = (c["dy"].double().abs() * (o["rstd"] * bm + rr * o["xh"].abs())).sum(0)  # d(dy xhat) from the statistics
    w["dgamma"] = within(f"{tag}.dgamma{sfx}", got["dgamma"], o["dgamma"],
                         bound_reduced(o["dgamma"], o["t_dgamma"], k, not params_fp32) + sg, check)
    if got.get("dbeta") is not None:
        w["dbeta"] = within(f"{tag}.dbeta{sfx}", got["dbeta"], o["dbeta"],
                            bound_reduced(o["dbeta"], o["t_dbeta"], k, not params_fp32), check)
    return w


# ------------------------------------------------------------------------------------ GroupNorm
def silu(z):
    return z * torch.sigmoid(z)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _rsqrt(v, dt):
    return v.rsqrt() if dt == F32 else 1.0 / v.sqrt()


def gn_stats(xe, G, eps, dt):
    """Two-pass mean and rstd per (n, g) of xe [N, C, P] (already in dt)."""
    N = xe.shape[0]
    xg = xe.reshape(N, G, -1)
    mean = xg.sum(-1) / xg.shape[-1]
    c = xg - mean[..., None]
    var = (c * c).sum(-1) / xg.shape[-1]
    return mean, _rsqrt(var + eps, dt)


def _per_channel(s, C, gmap=None):
    """[N, G] statistics -> [N, C, 1]; ``gmap`` (a planted error) overrides channel -> group."""
    G = s.shape[1]
    idx = torch.arange(C) // (C // G) if gmap is None else gmap
    return s[:, idx][..., None]


def gn_fwd(x, G, gamma, beta, eps=EPS, silu_on=False, add=None, dt=F64, folded=False, stats=None):
    """GroupNorm (+SiLU) of x [N, C, P] (+ add[n, c]) in any layout-free form: y [N, C, P], mean and
    rstd [N, G]. ``stats``: (mean, rstd) from elsewhere (the chunked emulation)."""
    N, C, P = x.shape
    xe = x.to(dt)
    a = add.to(dt)[:, :, None] if add is not None else None
    mean, rstd = stats if stats is not None else gn_stats(xe + a if a is not None else xe, G, eps, dt)
    mc, rc = _per_channel(mean, C), _per_channel(rstd, C)
    gw = gamma.to(dt)[None, :, None]
    gb = beta.to(dt)[None, :, None] if beta is not None else torch.zeros((), dtype=dt)
    if folded:  # y = x * scale + shift, shift = beta + (add - mean) * scale
        sc = rc * gw
        z = xe * sc + (gb + ((a if a is not None else 0.0) - mc) * sc)
    else:
        z = ((xe + a if a is not None else xe) - mc) * rc * gw + gb
    return {"y": silu(z) if silu_on else z, "mean": mean, "rstd": rstd,
            "stat": stat_terms_y(rc, gw, z - gb, silu_on)}


def gn_bwd(dy, x, G, gamma, beta, eps=EPS, silu_on=False, dt=F64, folded=False, gmap=None):
    """dz = dy silu'(z); dx = rstd (gamma dz - m1 - xhat m2) with m1, m2 the group means of gamma dz
    and gamma dz xhat; dw = sum_{n, p} dz xhat; db = sum_{n, p} dz."""
    N, C, P = x.shape
    xe, dyv = x.to(dt), dy.to(dt)
    mean, rstd = gn_stats(xe, G, eps, dt)
    mc, rc = _per_channel(mean, C, gmap), _per_channel(rstd, C, gmap)
    gw = gamma.to(dt)[None, :, None]
    gb = beta.to(dt)[None, :, None] if beta is not None else torch.zeros((), dtype=dt)
    xh = (xe - mc) * rc
    dz = dyv * dsilu(xh * gw + gb) if silu_on else dyv
    gy = dz * gw
    L = (C // G) * P
    m1 = _per_channel(gy.reshape(N, G, -1).sum(-1) / L, C)
    m2 = _per_channel((gy * xh).reshape(N, G, -1).sum(-1) / L, C)
    if folded:  # dx = sc dz + B x + Cc, B = -rstd^2 m2, Cc = rstd (rstd m2 mean - m1)
        dx = (rc * gw) * dz + ((-rc * rc * m2) * xe + rc * (rc * m2 * mc - m1))
    else:
        dx = rc * (gy - m1 - xh * m2)
    # with SiLU dz itself depends on z = xhat gamma + beta: |silu''| <= 1/2
    extra = (rc * gw.abs() * dyv.abs() * 0.5 * gw.abs() * rc, rc * gw.abs() * dyv.abs() * 0.5 * (gw * xh).abs()) if silu_on else None
    return {"dx": dx, "dw": (dz * xh).sum((0, 2)), "db": dz.sum((0, 2)),
            "t_dw": (dz.abs() * (xe.abs() + mc.abs()) * rc).sum((0, 2)), "t_db": dz.abs().sum((0, 2)),
            "stat": stat_terms_dx(rc, xh, m1, m2, dx, extra), "rc": rc, "xh": xh, "dz": dz, "gw": gw}


def dense_from_phase(ph, hw, swap=False):
    """ops.norms.phase_to_dense on [N, 4C, H/2+1, W/2+1]; ``swap`` plants the (a, b) <-> (b, a) error."""
    from kubernetes_cloud_amd.ops.norms import phase_to_dense
    if not swap:
        return phase_to_dense(ph, hw)
    C = ph.shape[1] // 4
    blocks = [ph[:, k * C:(k + 1) * C] for k in range(4)]
    return phase_to_dense(torch.cat([blocks[0], blocks[2], blocks[1], blocks[3]], 1), hw)


def dense_to_phase(x, fill):
    """A phase-layout tensor whose dense form is x [N, C, H, W]; the cells no phase reads hold
    ``fill`` (a poison: the kernel must not read them)."""
    N, C, H, W = x.shape
    ph = torch.full((N, 4 * C, H // 2 + 1, W // 2 + 1), fill, dtype=x.dtype)
    for a in range(2):
        for b in range(2):
            k = 2 * a + b
            ph[:, k * C:(k + 1) * C, a:a + H // 2, b:b + W // 2] = x[:, :, a::2, b::2]
    return ph


def cat_inputs(x1, x2, x1_add=None, phase_hw=None, swap=False):
    """The concat the kernel normalises as (x [N, C, P] float64 exact, add [N, C] fp32 or None, raw
    bf16 [N, C, P]): raw is the concat itself, rounded once where x1_add is present."""
    d1 = dense_from_phase(x1, phase_hw, swap) if phase_hw is not None else x1
    N, C1 = d1.shape[:2]
    C2 = x2.shape[1]
    cat = torch.cat([d1.reshape(N, C1, -1), x2.reshape(N, C2, -1)], 1)
    add = None
    raw = cat
    if x1_add is not None:
        add = torch.zeros(N, C1 + C2, dtype=F32)
        add[:, :C1] = x1_add.float()
        raw = (cat.float() + add[:, :, None]).to(BF16)  # one fp32 add of a bf16 and an fp32: one rounding
    return cat, add, raw


# ---- host geometry of the kernels, restated so a case can assert the arm it is named after
def nchw_geometry(N, C, hw, G):
    cpg = C // G
    NG, Lg = N * G, cpg * hw
    S = min((2048 + NG - 1) // NG, cpg, max(1, Lg // 8192))
    S = max(S, 1)
    SL = (Lg + S - 1) // S
    if hw % 8 == 0:
        SL = (SL + 7) // 8 * 8
    S = (Lg + SL - 1) // SL
    if hw % 8 == 0:
        bwd = "v256" if hw >= 2048 else "v64"
    else:
        bwd = "s256" if hw >= 2048 else ("s128" if hw >= 512 else "s64")
    return {"S": S, "SL": SL, "Lg": Lg, "cpg": cpg, "vec_stats": SL % 8 == 0 and Lg % 8 == 0,
            "vec_apply": SL % 8 == 0 and hw % 8 == 0, "staged": cpg <= 128, "bwd": bwd}


def nhwc_geometry(N, C, P, G):
    CH = max(64, (P + 63) // 64)
    cv = C // 8
    slabs = (cv + 255) // 256
    w = (cv + slabs - 1) // slabs
    R = min(64, 256 // w)
    nch = (P + CH - 1) // CH
    return {"CH": CH, "nchunks": nch, "last": P - (nch - 1) * CH, "slabs": slabs, "w": w, "R": R,
            "dead": slabs * w - cv, "rows": N * nch, "cg": C // G}


def nchw_chain(N, hw, bwd):
    """gn_plane_grads(_v): a thread's loop over its share of the plane, the 6 wave shuffles, the waves
    of a workgroup; gn_param_grads: N planes in sequence."""
    th = int(bwd[1:])
    per = -(-(hw // 8) // th) * 8 if bwd[0] == "v" else -(-hw // th)
    return per + 6 + th // 64 + N + K_TERM


def nchw_stat_chain(geo) -> int:
    """gn_slice_stats: a thread's share of the slice, then Welford merges (four roundings each)
    through 6 wave shuffles, 4 waves and the S slices; the division."""
    v = 8 if geo["vec_stats"] else 1
    return -(-geo["SL"] // (256 * v)) * v + 4 * (6 + 4 + geo["S"]) + 1


def nhwc_stat_chain(geo) -> int:
    """nhwc_chunk_stats: a thread's pixels of the chunk and the R rows through LDS; nhwc_group_stats:
    ceil(nchunks cg / 256) merges in a thread and 8 in the tree, four roundings each; the division."""
    return -(-geo["CH"] // geo["R"]) + geo["R"] + 4 * (-(-geo["nchunks"] * geo["cg"] // 256) + 8) + 1


def nhwc_chain(N, P, C, G):
    """nhwc_chunk_grads: a thread's pixels of the chunk (ceil(CH / R)), the R rows through LDS;
    nhwc_chan_grads: ceil(rows / 16) at most in one accumulator, 2 to fold the four, 16 row groups."""
    g = nhwc_geometry(N, C, P, G)
    return -(-g["CH"] // g["R"]) + g["R"] + -(-g["rows"] // 16) + 2 + 16 + K_TERM


def gn_flat_marks(geo, hw):
    """Indices into a group's cpg * hw contiguous elements (NCHW): first and last of the group, both
    sides of every plane boundary, of every slice boundary, and of the first and last 16-byte vector."""
    Lg = geo["Lg"]
    m = {0, 7, 8, Lg - 9, Lg - 8, Lg - 1}
    for k in range(1, geo["cpg"]):
        m |= {k * hw - 1, k * hw}
    for k in range(1, geo["S"]):
        m |= {k * geo["SL"] - 1, k * geo["SL"]}
    return sorted(i for i in m if 0 <= i < Lg)


def gn_cp_marks(geo, C, P, extra_c=()):
    """(channels, pixels) for channels-last: first / last pixel and both sides of every chunk boundary;
    first / last channel and both sides of the vector, group and slab boundaries (and ``extra_c``:
    C1 - 1 | C1 of the concat)."""
    ps = {0, P - 1}
    for k in range(1, geo["nchunks"]):
        ps |= {k * geo["CH"] - 1, k * geo["CH"]}
    cs = {0, 7, 8, C - 1, geo["cg"] - 1, geo["cg"], geo["w"] * 8 - 1, geo["w"] * 8, *extra_c}
    return sorted(c for c in cs if 0 <= c < C), sorted(p for p in ps if 0 <= p < P)


def gn_cases(N, C, G, P, flat_marks=None, cp_marks=None, last_chunk=None, bias=True, seed=0):
    """{name: case}; a case holds x, dy [N, C, P] bf16 and gamma, beta. ``last_chunk``: first pixel of
    the last pixel chunk (channels-last): the constant case also gets a variant whose last chunk alone
    is constant."""
    g = _gen(seed * 1000003 + N * 7919 + C * 131 + P)
    gamma, b = _params(C, g, bias)
    cg = C // G

    def mk(x, dy):
        return {"x": x.to(BF16), "dy": dy.to(BF16), "gamma": gamma, "beta": b, "N": N, "C": C, "G": G, "P": P}

    def rn():
        return torch.randn(N, C, P, generator=g)

    out = {"uniform": mk(rn(), rn()), "offset": mk(50.0 + rn(), rn())}
    if cg > 1:  # one channel of every group at +40, the rest near 0: the merge term d^2 n n2 / nt is the variance
        x = 0.25 * rn()
        x[:, ::cg] += 40.0
        out["offset-channel"] = mk(x, rn())
    out["constant"] = mk(torch.full((N, C, P), 1.5), rn())
    if last_chunk is not None:
        x = rn()
        x[:, :, last_chunk:] = 1.5
        out["constant-last-chunk"] = mk(x, rn())
    x, dy = TINY * rn(), TINY * rn()
    if flat_marks is not None:
        m = torch.tensor(flat_marks)
        sign = torch.where(torch.arange(m.numel()) % 2 == 0, BIG, -BIG)
        xv, dv = x.view(N, G, -1), dy.view(N, G, -1)
        xv[:, :, m] = sign
        dv[:, :, m] = sign.flip(0)
    if cp_marks is not None:
        cs, ps = (torch.tensor(t) for t in cp_marks)
        sign = torch.where((cs[:, None] + ps[None, :]) % 2 == 0, BIG, -BIG)
        x[:, cs[:, None], ps[None, :]] = sign
        dy[:, cs[:, None], ps[None, :]] = -sign
    out["planted"] = mk(x, dy)
    return out


def poison_group(x, G, n, g):
    """x [N, C, P] with group (n, g) holding NaN, +inf and -inf."""
    N, C, P = x.shape
    v = x.clone().view(N * G, -1)
    return poison_rows(v, n * G + g).view(N, C, P)


def check_gn_fwd(tag, c, got, silu_on, ks, add=None, x64=None, check=True):
    """got: y [N, C, P], mean, rstd [N, G]. ks: nchw_stat_chain / nhwc_stat_chain of the case.
    ``x64``: the exact input where it is not c["x"] (concat)."""
    x = c["x"] if x64 is None else x64
    G = c["G"]
    xa = x.double() + (add.double()[:, :, None] if add is not None else 0.0)
    am = xa.abs().reshape(x.shape[0], G, -1).mean(-1)
    o = gn_fwd(x, G, c["gamma"], c["beta"], silu_on=silu_on, add=add)
    e = gn_fwd(x, G, c["gamma"], c["beta"], silu_on=silu_on, add=add, dt=F32, folded=True)
    N = x.shape[0]
    grp = lambda t: t.reshape(N, G, -1)  # noqa: E731
    bm, br = bound_mean(am, ks), bound_rstd(o["rstd"], ks)
    by = bound_bf16(grp(o["y"]), grp(e["y"]), -1) + grp(o["stat"][0] * _per_channel(bm, x.shape[1])
                                                         + o["stat"][1] * _per_channel(br / o["rstd"], x.shape[1]))
    w = {"y": within(f"{tag}.y", grp(got["y"]), grp(o["y"]), by, check)}
    if got.get("mean") is not None:
        w["mean"] = within(f"{tag}.mean", got["mean"].reshape(N, G), o["mean"], bm, check)
        w["rstd"] = within(f"{tag}.rstd", got["rstd"].reshape(N, G), o["rstd"], br, check)
    return w


def check_gn_bwd(tag, c, got, silu_on, k, ks, folded, check=True):
    """got: dx [N, C, P], dw, db (None without bias). k: nchw_chain / nhwc_chain of the case; ks: its
    statistics chain (the backward is handed the forward's fp32 mean and rstd)."""
    G, N, C = c["G"], c["N"], c["C"]
    o = gn_bwd(c["dy"], c["x"], G, c["gamma"], c["beta"], silu_on=silu_on)
    e = gn_bwd(c["dy"], c["x"], G, c["gamma"], c["beta"], silu_on=silu_on, dt=F32, folded=folded)
    grp = lambda t: t.reshape(N, G, -1)  # noqa: E731
    bm = _per_channel(bound_mean(c["x"].double().abs().reshape(N, G, -1).mean(-1), ks), C)
    rr = bound_rstd(1.0, ks)
    bdx = bound_bf16(grp(o["dx"]), grp(e["dx"]), -1) + grp(o["stat"][0] * bm + o["stat"][1] * rr)
    dxh = o["rc"] * bm + rr * o["xh"].abs()  # what the statistics' error does to xhat
    sw = (o["dz"].abs() * dxh).sum((0, 2))
    sb = torch.zeros_like(sw)
    if silu_on:  # and through silu' to dz
        ddz = c["dy"].double().abs() * 0.5 * o["gw"].abs() * dxh
        sw, sb = sw + (ddz * o["xh"].abs()).sum((0, 2)), ddz.sum((0, 2))
    w = {"dx": within(f"{tag}.dx", grp(got["dx"]), grp(o["dx"]), bdx, check),
         "dw": within(f"{tag}.dw", got["dw"], o["dw"], bound_reduced(o["dw"], o["t_dw"], k, True) + sw, check)}
    if got.get("db") is not None:
        w["db"] = within(f"{tag}.db", got["db"], o["db"], bound_reduced(o["db"], o["t_db"], k, True) + sb, check)
    return w


# ------------------------------------------------------------------------------------ fp32 emulation of the chunked statistics
def chan_merge(n, mu, m2, n2, mu2, q2):
    nt = n + n2
    d = mu2 - mu
    return nt, mu + d * n2 / nt, m2 + q2 + d * d * n * n2 / nt


def _partial(v, dt):
    """(mean, M2) over the last dim, two-pass, in dt."""
    mean = v.sum(-1) / v.shape[-1]
    c = v - mean[..., None]
    return mean, (c * c).sum(-1)


def stats_sliced(x, G, SL, eps=EPS, dt=F32, mut=None):
    """groupnorm.hip's forward statistics: each (n, g) group's contiguous elements cut into slices of
    SL, a (mean, M2) partial per slice, Chan merge in sequence with n2 = min(SL, Lg - k SL).
    mut "slice-count": n2 = SL for the last slice too."""
    N = x.shape[0]
    xg = x.to(dt).reshape(N, G, -1)
    Lg = xg.shape[-1]
    n = torch.zeros(N, G, dtype=dt)
    mu, m2 = torch.zeros_like(n), torch.zeros_like(n)
    for a in range(0, Lg, SL):
        pm, pq = _partial(xg[..., a:min(a + SL, Lg)], dt)
        n2 = float(SL if mut == "slice-count" else min(SL, Lg - a))
        n, mu, m2 = chan_merge(n, mu, m2, n2, pm, pq)
    return mu, _rsqrt(m2 / n + eps, dt)


def stats_chunked(x, G, CH, add=None, eps=EPS, dt=F32, mut=None):
    """groupnorm_nhwc.hip's: a (mean, M2) partial per (n, pixel chunk, channel), Chan merge over the
    chunks x channels of a group, the per-(n, c) add shifting each partial's mean.
    mut "chunk-count": the last chunk counted as CH pixels; "no-add": add left out of the statistics."""
    N, C, P = x.shape
    cg = C // G
    xe = x.to(dt)
    n = torch.zeros(N, G, dtype=dt)
    mu, m2 = torch.zeros_like(n), torch.zeros_like(n)
    sh = add.to(dt) if (add is not None and mut != "no-add") else torch.zeros(N, C, dtype=dt)
    for p0 in range(0, P, CH):
        pm, pq = _partial(xe[:, :, p0:min(p0 + CH, P)], dt)  # [N, C]
        cn = float(CH if mut == "chunk-count" else min(CH, P - p0))
        pm = pm + sh
        for j in range(cg):
            n, mu, m2 = chan_merge(n, mu, m2, cn, pm.view(N, G, cg)[..., j], pq.view(N, G, cg)[..., j])
    return mu, _rsqrt(m2 / n + eps, dt)


# ------------------------------------------------------------------------------------ the shapes under test
# LayerNorm: (rows, d, [(nres, beta, dres, params_fp32), ...], forward only)
LN_SHAPES = [
    (5, 8, [(0, True, False, 0), (2, False, True, 1)], False),          # one vector, 63 idle lanes
    (3, 16384, [(1, True, True, 0)], False),                            # NV = 8, the widest row
    (1, 2056, [(0, True, False, 1)], False),                            # NV = 2 with one vector in the second pass
    (257, 2048, [(2, True, True, 0), (0, False, False, 0)], False),
    (4099, 72, [(0, True, False, 0)], False),                           # narrow NV = 1, 3 rows into a second pass
    (4099, 520, [(1, True, True, 1)], False),                           # narrow NV = 2
    (1025, 512, [(0, True, False, 0)], False),                          # 1024 parts through col_reduce64
    (1023, 1024, [(2, True, True, 1)], False),
    (2051, 1032, [(0, True, False, 0), (1, False, True, 1)], False),    # block kernel, 2-3 rows per workgroup
    (262143, 8, [(0, True, False, 0), (1, False, False, 0)], True),     # grid-stride second pass of the forward
]

# NCHW GroupNorm: (N, C, G, H, W) -> what nchw_geometry must say
NCHW_SHAPES = [
    ((1, 40, 8, 5, 7), dict(S=1, vec_stats=False, vec_apply=False, staged=True, bwd="s64")),
    ((2, 20, 2, 6, 6), dict(S=1, vec_stats=True, vec_apply=False, staged=True, bwd="s64")),
    ((1, 10, 2, 27, 152), dict(S=2, SL=10264, vec_stats=True, vec_apply=True, staged=True, bwd="v256")),
    ((1, 266, 2, 8, 8), dict(S=1, vec_stats=True, vec_apply=True, staged=False, bwd="v64")),
    ((3, 6, 6, 47, 47), dict(S=1, vec_stats=False, vec_apply=False, staged=True, bwd="s256")),
    ((1, 8, 1, 23, 23), dict(S=1, vec_stats=True, vec_apply=False, staged=True, bwd="s128")),
    ((1, 4, 1, 65, 65), dict(S=2, SL=8450, vec_stats=False, vec_apply=False, staged=True, bwd="s256")),
    ((1, 8, 1, 42, 50), dict(S=2, SL=8400, vec_stats=True, vec_apply=False, staged=True, bwd="s256")),
]

# channels-last GroupNorm: (N, C, G, H, W) -> what nhwc_geometry must say
NHWC_SHAPES = [
    ((1, 8, 1, 1, 1), dict(nchunks=1, last=1, slabs=1, R=64)),
    ((2, 40, 4, 5, 7), dict(nchunks=1, last=35, cg=10)),
    ((1, 80, 8, 5, 13), dict(nchunks=2, last=1, cg=10)),
    ((1, 16, 2, 37, 109), dict(CH=64, nchunks=64, last=1)),
    ((1, 16, 2, 17, 241), dict(CH=65, nchunks=64, last=2)),
    ((1, 2056, 8, 3, 3), dict(slabs=2, R=1, w=129, dead=1)),
    ((3, 16, 2, 35, 40), dict(rows=66, nchunks=22)),
    ((3, 320, 32, 4, 4), dict(nchunks=1, cg=10, R=6)),
]


def assert_geometry(geo: dict, want: dict, what):
    for k, v in want.items():
        assert geo[k] == v, (what, k, geo[k], v, geo)
