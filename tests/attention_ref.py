"""float64 oracle, input generators and per-element bounds for the flash-attention kernels
(csrc/kernels/attention.hip, attention_tiled.hip).

The oracles are written from the formulas in attention.hip's header comment in plain float64 torch and
do not call ops.attention_reference. tests/test_attention_ref_cpu.py pins them against
F.scaled_dot_product_attention (fp64, autograd) and ops.attention_reference, shows that a CPU
emulation of the kernels' arithmetic meets every bound below, and that every planted edge is at least
16 bounds tall; tests/test_attention_elem_gpu.py applies the same generators and bounds to the HIP
kernels. Inputs are generated on the CPU from a seed, so both files see the same numbers.

Layouts are the kernels': q, o, do, dq [B, Sq, H, D]; k, v, dk, dv [B, Sk, Hkv, D]; lse [B, H, Sq];
p, ds [B, H, Sq, Sk].
"""
from __future__ import annotations

import math

import torch

from . import train_tail_ref as _T
from .train_tail_ref import WORST, Guarded, bits_equal  # noqa: F401  (re-exported)

U = 2.0 ** -8  # bf16 unit roundoff (round to nearest: half the spacing of 2^-7)
LOG2E = 1.4426950408889634
# The leading 2u (P or dS rounded to bf16, the result rounded to bf16) is fixed; (1 + 2^-6) lets the
# two roundings compound and covers the fp32 accumulation of at most 512 terms.
LEAD = 2 * U * (1 + 2.0 ** -6)
EPS_P_UNIT = 2.0 ** -18   # relative error of one probability per unit of max_k scale * sum_d |q_d k_d|
EPS_DP_UNIT = 2.0 ** -20  # fp32 accumulation error of do.v and of delta, per unit of their magnitude sums
DO_GAIN = 4.0             # weight of the planted v_j in do_i (make_inputs)
SENSITIVITY = 16.0        # a planted pair, taken out, must move every output by this many bounds


def assert_within(name, actual, expected64, bound64):
    """train_tail_ref.assert_within under this file's own print prefix."""
    return _T.assert_within(name, actual, expected64, bound64, prefix="attention")


# ------------------------------------------------------------------------------------ masks
def attend_mask(B, H, Sq, Sk, causal, kv_len=None, key_mask=None, window=0):
    """bool [B, H, Sq, Sk], True where query q attends to key k. causal is bottom-right aligned
    (key <= q + Sk - Sq); kv_len int [B] (key < kv_len[b]); key_mask bool [B, Sk] (True = attend);
    window > 0: key > q + Sk - Sq - window."""
    qi = torch.arange(Sq)[:, None]
    ki = torch.arange(Sk)[None, :]
    off = Sk - Sq
    att = torch.ones(B, H, Sq, Sk, dtype=torch.bool)
    if causal:
        att &= (ki <= qi + off)
    if window:
        att &= (ki > qi + off - window)
    if kv_len is not None:
        att &= (ki[None, None] < torch.as_tensor(kv_len).view(B, 1, 1, 1))
    if key_mask is not None:
        att &= key_mask.view(B, 1, 1, Sk)
    return att


def excluded_keys(B, Sk, kv_len=None, key_mask=None):
    """bool [B, Sk]: keys the per-key masks exclude for every query."""
    ex = torch.zeros(B, Sk, dtype=torch.bool)
    if kv_len is not None:
        ex |= torch.arange(Sk)[None] >= torch.as_tensor(kv_len).view(B, 1)
    if key_mask is not None:
        ex |= ~key_mask
    return ex


def _heads(q, k, v):
    """fp64 [B, H, S, D] copies, K/V repeated over the query heads of their group."""
    H, Hkv = q.shape[2], k.shape[2]
    qd = q.detach().double().cpu().permute(0, 2, 1, 3)
    kd = k.detach().double().cpu().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    vd = v.detach().double().cpu().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    return qd, kd, vd


def _scores(qd, kd, scale, alibi):
    """(scores, magnitude sums scale * sum_d |q_d k_d| + |alibi term|), both [B, H, Sq, Sk]."""
    Sq, Sk = qd.shape[2], kd.shape[2]
    s = scale * (qd @ kd.transpose(-1, -2))
    mag = abs(scale) * (qd.abs() @ kd.abs().transpose(-1, -2))
    if alibi is not None:
        dist = (torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] - (Sk - Sq)).double()
        bias = alibi.detach().double().cpu().view(1, -1, 1, 1) * dist
        s = s + bias
        mag = mag + bias.abs()
    return s, mag


def _eps_p(mag, att):
    """[B, H, Sq]: 2^-18 * max(1, largest score magnitude sum among the attended keys of the row). A
    masked key's score never reaches an exponential in any kernel, so it does not count."""
    return EPS_P_UNIT * mag.masked_fill(~att, 0.0).amax(-1).clamp_min(1.0)


def _group_sum(x, Hkv):
    """[B, H, Sk, D] -> [B, Sk, Hkv, D], summed over the query heads of each KV head."""
    B, H, Sk, D = x.shape
    return x.view(B, Hkv, H // Hkv, Sk, D).sum(2).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------ oracles
def fwd(q, k, v, causal, scale, kv_len=None, key_mask=None, alibi=None, window=0, attend=None):
    """softmax(scale q k^T + alibi + mask) v in float64. ``attend`` replaces the mask built from the
    arguments (the sensitivity checks edit one). Returns a dict: o [B, Sq, H, D]; lse [B, H, Sq]
    (natural log, +inf for a row with no key); p; A_o = sum_k p |v|; eps_p [B, H, Sq]; bound_o;
    bound_lse; attend."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qd, kd, vd = _heads(q, k, v)
    s, mag = _scores(qd, kd, scale, alibi)
    att = attend if attend is not None else attend_mask(B, H, Sq, Sk, causal, kv_len, key_mask, window)
    s = s.masked_fill(~att, -math.inf)
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    some = l > 0
    p = torch.where(some, e / torch.where(some, l, torch.ones_like(l)), torch.zeros_like(e))
    lse = torch.where(some, mx + torch.log(torch.where(some, l, torch.ones_like(l))),
                      torch.full_like(l, math.inf)).squeeze(-1)
    eps_p = _eps_p(mag, att)
    o = (p @ vd).permute(0, 2, 1, 3)
    A_o = (p @ vd.abs()).permute(0, 2, 1, 3)
    bound_o = (LEAD + 2 * eps_p).permute(0, 2, 1)[..., None] * A_o
    fin = torch.where(some.squeeze(-1), lse.abs(), torch.zeros_like(lse))
    bound_lse = 2 * eps_p + 2.0 ** -22 * (Sk + 8 * fin.clamp_min(1.0))
    return dict(o=o, lse=lse, p=p, A_o=A_o, eps_p=eps_p, bound_o=bound_o, bound_lse=bound_lse, attend=att)


def bwd(q, k, v, o, lse, do, causal, scale, kv_len=None, key_mask=None, alibi=None, window=0, attend=None):
    """The function the backward kernels implement, in float64, from the STORED o (bf16) and lse (fp32):
    p = exp(s - lse), delta = sum_d do o, ds = p (do v^T - delta), dv = p^T do, dk = scale ds^T q,
    dq = scale ds k; dk, dv summed over the query heads of a group. Returns a dict with dq, dk, dv,
    p, ds, A_dv = sum_q p |do| and the bounds bound_dq, bound_dk, bound_dv."""
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qd, kd, vd = _heads(q, k, v)
    od = o.detach().double().cpu().permute(0, 2, 1, 3)
    dod = do.detach().double().cpu().permute(0, 2, 1, 3)
    lsed = lse.detach().double().cpu()
    s, mag = _scores(qd, kd, scale, alibi)
    att = attend if attend is not None else attend_mask(B, H, Sq, Sk, causal, kv_len, key_mask, window)
    p = torch.exp(s.masked_fill(~att, -math.inf) - lsed[..., None])  # lse = +inf: exp(-inf) = 0
    p = torch.where(att, p, torch.zeros_like(p))
    delta = (dod * od).sum(-1, keepdim=True)
    dp = dod @ vd.transpose(-1, -2)
    ds = p * (dp - delta)
    dv = _group_sum(p.transpose(-1, -2) @ dod, Hkv)
    dk = scale * _group_sum(ds.transpose(-1, -2) @ qd, Hkv)
    dq = scale * (ds @ kd).permute(0, 2, 1, 3)
    eps_p = _eps_p(mag, att)[..., None]
    eps_dp = EPS_DP_UNIT * (dod.abs() @ vd.abs().transpose(-1, -2) + (dod * od).abs().sum(-1, keepdim=True))
    e_ds = (U * (1 + 2.0 ** -6) + 2 * eps_p) * ds.abs() + p * eps_dp
    A_dv = _group_sum(p.transpose(-1, -2) @ dod.abs(), Hkv)
    bound_dv = _group_sum((p * (LEAD + 2 * eps_p)).transpose(-1, -2) @ dod.abs(), Hkv)
    bound_dk = abs(scale) * _group_sum(e_ds.transpose(-1, -2) @ qd.abs(), Hkv) * (1 + 2.0 ** -7) + U * dk.abs()
    bound_dq = (abs(scale) * (e_ds @ kd.abs()) * (1 + 2.0 ** -7)).permute(0, 2, 1, 3) + U * dq.abs()
    return dict(dq=dq, dk=dk, dv=dv, p=p, ds=ds, A_dv=A_dv, bound_dq=bound_dq, bound_dk=bound_dk,
                bound_dv=bound_dv, attend=att)


# ------------------------------------------------------------------------------------ CPU emulation
def emulate_fwd(q, k, v, scale, att, alibi=None):
    """The kernels' arithmetic in CPU torch: fp32 scores in log2 units, exp2, P rounded to bf16 before
    the second product, fp32 accumulation, one bf16 rounding of o. Returns (o bf16, lse fp32)."""
    H, Hkv = q.shape[2], k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    Sq, Sk = qf.shape[2], kf.shape[2]
    x = (qf @ kf.transpose(-1, -2)) * torch.tensor(scale * LOG2E, dtype=torch.float32)
    if alibi is not None:
        dist = (torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] - (Sk - Sq)).float()
        x = x + (alibi.float() * torch.tensor(LOG2E, dtype=torch.float32)).view(1, -1, 1, 1) * dist
    x = x.masked_fill(~att, -math.inf)
    m = x.amax(-1, keepdim=True)
    m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp2(x - m0)
    l = e.sum(-1, keepdim=True)
    pb = e.bfloat16().float()
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o = ((pb @ vf) * inv).permute(0, 2, 1, 3).bfloat16()
    lse = torch.where(l > 0, (m0 + torch.log2(l)) * torch.tensor(math.log(2.0), dtype=torch.float32),
                      torch.full_like(l, math.inf)).squeeze(-1)
    return o, lse


def emulate_bwd(q, k, v, o, lse, do, scale, att, alibi=None):
    """Backward twin of emulate_fwd: fp32 p = exp2(s log2e - lse log2e), fp32 do.v and delta, P and dS
    rounded to bf16, fp32 accumulation, bf16 results. Returns (dq, dk, dv) bf16."""
    B, Sq, H, D = q.shape
    Hkv = k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
    of = o.float().permute(0, 2, 1, 3)
    gf = do.float().permute(0, 2, 1, 3)
    Sk = kf.shape[2]
    l2e = torch.tensor(LOG2E, dtype=torch.float32)
    x = (qf @ kf.transpose(-1, -2)) * torch.tensor(scale * LOG2E, dtype=torch.float32) - (lse.float() * l2e)[..., None]
    if alibi is not None:
        dist = (torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] - (Sk - Sq)).float()
        x = x + (alibi.float() * l2e).view(1, -1, 1, 1) * dist
    p = torch.where(att, torch.exp2(x), torch.zeros_like(x))
    delta = (gf * of).sum(-1, keepdim=True)
    ds = p * (gf @ vf.transpose(-1, -2) - delta)
    pb, dsb = p.bfloat16().float(), ds.bfloat16().float()
    sc = torch.tensor(scale, dtype=torch.float32)
    dv = _group_sum(pb.transpose(-1, -2) @ gf, Hkv).bfloat16()
    dk = (_group_sum(dsb.transpose(-1, -2) @ qf, Hkv) * sc).bfloat16()
    dq = ((dsb @ kf) * sc).permute(0, 2, 1, 3).bfloat16()
    return dq, dk, dv


# ------------------------------------------------------------------------------------ generators
def diagonal_pairs(Sq, Sk, H, Hkv):
    """Default planted pairs (h, i, j): the bottom-right diagonal j = i + Sk - Sq. With GQA key j is
    planted for query head hk * grp + j % grp only, so every query head of a group owns keys of its
    own and a head left out of the dK/dV sweep shows."""
    grp = H // Hkv
    out = []
    for i in range(Sq):
        j = i + Sk - Sq
        if 0 <= j < Sk:
            out += [(hk * grp + j % grp, i, j) for hk in range(Hkv)]
    return out


def tile_edge_keys(Sk):
    """First and last key of every 32-key tile (which includes every 64- and 128-key block edge)."""
    return [j for j in range(Sk) if j % 32 in (0, 31)] + [Sk - 1]


def make_inputs(seed, B, Sq, Sk, H, Hkv, D, kind="peaked", pairs=None, excluded=None, q_gain=None, attend=None,
                scale=None, bias=None):
    """(q, k, v, do) bf16 on the CPU. ``attend`` is the case's mask [B, H, Sq, Sk] (default: all), ``bias``
    its ALiBi term [1, H, Sq, Sk] or None.
    ``uniform``: randn; exercises rounding only.
    ``peaked``: for every (h, i, j) of ``pairs`` (all batches; a key planted twice keeps the last;
    default diagonal_pairs):
      k[j] <- 3 q[i] + 0.3 k[j], so that p_ij dominates row i of head h;
      q[i] is scaled to |q_i|^2 = D gain^2 with gain = peak_gain(keys row i attends to, counted with
        their ALiBi weights), per batch row (``q_gain`` overrides both), so that p_ij is near 0.8 whether the row sees 2 keys or 500: at p = 1 the row has no gradient;
      do[i] += +-DO_GAIN v[j] where the pair is attended, the sign alternating over the planted keys
        of one row. The pair's dS = p_ij do_i . (v_j - o_i) is then about DO_GAIN p (1 - p) |v_j|^2
        instead of a random scalar that can lie near zero, and with alternating signs it stays
        large when two planted keys share a row (same signs cancel as p_1 + p_2 -> 1);
      a row without an attended planted pair (its diagonal key lies past kv_len, in a hole, or
        belongs to another head of its group) has do scaled by 1/8: it still has a checked,
        non-zero dq, but does not drown the planted rows in the bounds of dk and dv, which sum
        over all rows.
    ``excluded`` bool [B, Sk] (poison): q's column 0 becomes 1 + |q_0| before the gain, and every
    excluded key gets K = 16 D e_0 -- a score above any planted one for every query -- and V = 2^20,
    so one leaked key is orders of magnitude above any bound. (No NaN: 0 * NaN is NaN in any
    implementation.)"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, H, D, generator=g)
    k = torch.randn(B, Sk, Hkv, D, generator=g)
    v = torch.randn(B, Sk, Hkv, D, generator=g)
    do = torch.randn(B, Sq, H, D, generator=g)
    if excluded is not None:
        q[..., 0] = 1.0 + q[..., 0].abs()
    if attend is None:
        attend = torch.ones(B, H, Sq, Sk, dtype=torch.bool)
    if q_gain is None:
        q_gain = 1.0
        if kind == "peaked":
            w = attend.double() if bias is None else attend * torch.exp(bias.double())
            n = w.sum(-1).clamp_min(2).permute(0, 2, 1)[..., None].float()   # [B, Sq, H, 1]
            q_gain = peak_gain(n, D, scale if scale is not None else D ** -0.5)
            q = q * (D ** 0.5 / q.norm(dim=-1, keepdim=True))  # |q_i|^2 = D: every planted score on target
    q = (q * q_gain).bfloat16()
    if kind == "peaked":
        grp = H // Hkv
        planted = torch.zeros(B, Sq, H, dtype=torch.long)
        for h, i, j in (pairs if pairs is not None else diagonal_pairs(Sq, Sk, H, Hkv)):
            k[:, j, h // grp] = 3.0 * q[:, i, h].float() + 0.3 * k[:, j, h // grp]
            live = attend[:, h, i, j]
            sign = (1 - 2 * (planted[:, i, h] % 2)).float() * live
            do[:, i, h] += DO_GAIN * sign[:, None] * v[:, j, h // grp]
            planted[:, i, h] += live
        do[planted == 0] *= 0.125
    elif kind != "uniform":
        raise ValueError(kind)
    if excluded is not None:
        pk = torch.zeros(D)
        pk[0] = 16.0 * D
        k[excluded] = pk
        v[excluded] = 2.0 ** 20
    return q, k.bfloat16(), v.bfloat16(), do.bfloat16()


def peak_gain(n_keys, D, scale):
    """Gain on q that puts a planted score, 3 scale |q_i|^2 = 3 scale D gain^2 on average, at
    ln(n_keys) + 2: the planted probability then dominates its row (about 0.8 among n_keys scores of
    unit size) without saturating it. At p_ij = 1 the row's softmax has no gradient (ds = 0), and a
    pair dropped by a backward kernel alone would move neither dk nor dq. ``n_keys``: int or tensor."""
    n = torch.as_tensor(n_keys, dtype=torch.float32)
    return ((torch.log(n) + 2.0) / (3.0 * D * scale)).clamp_max(1.0).sqrt()


# ------------------------------------------------------------------------------------ sensitivity
def pair_sensitivity(q, k, v, do, scale, f, b_, pairs):
    """For every planted pair (h, i, j): the largest |change| / bound at one element of o, dv, dk and
    dq when that pair alone is taken out of the mask. ``f`` and ``b_`` are the dicts of fwd() and
    bwd(). Row i of o becomes (o_i - p_ij v_j) / (1 - p_ij); with the stored lse the backward changes
    by exactly the pair's own terms: dv_j -= p_ij do_i, dk_j -= scale ds_ij q_i, dq_i -= scale ds_ij
    k_j. Returns float64 [4, B, len(pairs)] in that order (inf where a bound is 0 and the change is
    not, 0 where neither is)."""
    grp = q.shape[2] // k.shape[2]
    h, i, j = (torch.tensor(x, dtype=torch.long) for x in zip(*pairs))
    hk = h // grp
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    pij = f["p"][:, h, i, j][..., None]            # [B, P, 1]
    dsij = b_["ds"][:, h, i, j][..., None]
    o_i = f["o"][:, i, h]                           # [B, P, D]
    rest = (1 - pij).clamp_min(1e-300)
    changes = [((o_i - pij * vd[:, j, hk]) / rest - o_i, f["bound_o"][:, i, h]),
               (pij * dod[:, i, h], b_["bound_dv"][:, j, hk]),
               (scale * dsij * qd[:, i, h], b_["bound_dk"][:, j, hk]),
               (scale * dsij * kd[:, j, hk], b_["bound_dq"][:, i, h])]
    out = []
    for d, bound in changes:
        d = d.abs()
        out.append(torch.where(d == 0, torch.zeros_like(d), d / bound).amax(-1))
    return torch.stack(out)


def window_pairs(Sq, Sk, H, W):
    """Window cases use four heads (H == Hkv): head 0 plants the last key of each row's window (the
    diagonal), head 1 the first (j = i + off - W + 1), head 2 the key just LEFT of the window
    (j = i + off - W) and head 3 the key just past the diagonal (j = i + off + 1) -- the last two
    are outside the mask, so a comparison that admits one key too many moves the row as far as
    dropping one does. Returns (inside pairs, outside pairs)."""
    off = Sk - Sq
    inside, outside = [], []
    for i in range(Sq):
        for h, j in ((0, i + off), (1, i + off - W + 1)):
            if 0 <= j < Sk and h < H:
                inside.append((h, i, j))
        for h, j in ((2, i + off - W), (3, i + off + 1)):
            if 0 <= j < Sk and h < H:
                outside.append((h, i, j))
    return inside, outside


def spread_pairs(Sq, Sk, H, Hkv, keys, causal):
    """One planted pair per key of ``keys``, spread round-robin over the rows that see the key and
    over the query heads of a group, so no row carries more than a few."""
    grp = H // Hkv
    off = Sk - Sq
    out = []
    for n, j in enumerate(sorted(set(keys))):
        if not 0 <= j < Sk:
            continue
        lo = min(max(j - off, 0), Sq - 1) if causal else 0
        i = lo + n % (Sq - lo)
        out += [(hk * grp + n % grp, i, j) for hk in range(Hkv)]
    return out


# ------------------------------------------------------------------------------------ cases
def case(name, Sq, Sk, D, causal, B=2, H=2, Hkv=None, **kw):
    c = dict(name=name, B=B, Sq=Sq, Sk=Sk, H=H, Hkv=Hkv or H, D=D, causal=causal, scale=None, kv_len=None,
             holes=None, alibi=False, window=0, kind="peaked", edges=None, q_gain=None)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    return c


def materialize(c):
    """Inputs and mask arguments of a case: dict(q, k, v, do, scale, kv_len, key_mask, alibi, window,
    pairs, outside, excluded, kw) -- kw are the oracle's keyword arguments."""
    import zlib
    B, Sq, Sk, H, Hkv, D = (c[n] for n in ("B", "Sq", "Sk", "H", "Hkv", "D"))
    kv_len = torch.tensor(c["kv_len"], dtype=torch.int32) if c["kv_len"] is not None else None
    key_mask = None
    if c["holes"] is not None:
        key_mask = torch.ones(B, Sk, dtype=torch.bool)
        for b, ks in enumerate(c["holes"]):
            key_mask[b, list(ks)] = False
    excluded = excluded_keys(B, Sk, kv_len, key_mask) if (kv_len is not None or key_mask is not None) else None
    outside = []
    if c["window"]:
        pairs, outside = window_pairs(Sq, Sk, H, c["window"])
    else:
        pairs = diagonal_pairs(Sq, Sk, H, Hkv)
        if c["edges"] is not None:
            pairs = pairs + spread_pairs(Sq, Sk, H, Hkv, c["edges"], c["causal"])
    # a key planted twice keeps the last pair: only that one is a planted pair
    grp = H // Hkv
    last = {(h // grp, j): (h, i, j) for h, i, j in pairs + outside}
    pairs = [t for t in dict.fromkeys(pairs) if last[(t[0] // grp, t[2])] == t]
    outside = [t for t in dict.fromkeys(outside) if last[(t[0] // grp, t[2])] == t]
    scale = c["scale"] if c["scale"] is not None else D ** -0.5
    attend = attend_mask(B, H, Sq, Sk, c["causal"], kv_len, key_mask, c["window"])
    alibi = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)]) if c["alibi"] else None  # BLOOM's
    bias = None
    if alibi is not None:
        bias = alibi.view(1, H, 1, 1) * (torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] - (Sk - Sq))
    q, k, v, do = make_inputs(zlib.crc32(c["name"].encode()), B, Sq, Sk, H, Hkv, D, c["kind"], pairs + outside,
                              excluded, c["q_gain"], attend, scale, bias)
    kw = dict(causal=c["causal"], scale=scale, kv_len=kv_len, key_mask=key_mask, alibi=alibi, window=c["window"])
    return dict(q=q, k=k, v=v, do=do, scale=scale, kv_len=kv_len, key_mask=key_mask, alibi=alibi,
                window=c["window"], pairs=pairs, outside=outside, excluded=excluded, kw=kw)


GENERIC_DIMS = [8, 40, 64, 72, 96, 128, 136, 160, 200, 256]  # pad to 64 64 64 96 96 128 160 160 256 256
S_ODD = 161  # two 128-row blocks, a partial last wave, a partial last 32-key tile and 64-key dK/dV block


def generic_cases():
    out = [case(f"generic-d{d}-{'causal' if ca else 'full'}", S_ODD, S_ODD, d, ca, edges=tile_edge_keys(S_ODD))
           for d in GENERIC_DIMS for ca in (False, True)]
    for d in (40, 128, 256):
        out.append(case(f"offset-37x300-d{d}", 37, 300, d, True, edges=tile_edge_keys(300)))
        out.append(case(f"decode-1x300-d{d}", 1, 300, d, True, edges=[0, 31, 32]))
        out.append(case(f"empty-rows-200x130-d{d}", 200, 130, d, True, edges=tile_edge_keys(130)))
    out.append(case("cross-37x300-d96", 37, 300, 96, False, edges=tile_edge_keys(300)))
    out.append(case("generic-gqa-d64", S_ODD, S_ODD, 64, True, H=4, Hkv=2, edges=tile_edge_keys(S_ODD)))
    out.append(case("generic-gqa-d256", S_ODD, S_ODD, 256, True, H=4, Hkv=2, edges=tile_edge_keys(S_ODD)))
    return out


def mask_cases():
    S = S_ODD
    out = []
    for n, (lens, ca, d) in enumerate([((0, S), True, 64), ((S - 1, 1), False, 64), ((31, 33), True, 64),
                                       ((32, S), False, 128), ((33, 0), True, 256), ((32, 31), False, 256)]):
        out.append(case(f"kvlen-{lens[0]}-{lens[1]}-d{d}", S, S, d, ca, kv_len=list(lens)))
    out.append(case("holes-31-32-63-64", S, S, 64, True, holes=[(31, 32), (63, 64)]))
    out.append(case("holes-31-32-63-64-full-d256", S, S, 256, False, holes=[(31, 32), (63, 64)]))
    out.append(case("holes-partial-word-77", 77, 77, 64, False, holes=[(64, 76), tuple(range(70, 77))]))
    out.append(case("holes-key0-causal", S, S, 64, True, holes=[(0,), (0, 1, 2)]))
    out.append(case("holes-key0-causal-d128", S, S, 128, True, holes=[(0, 1), (0,)]))
    for w in (1, 31, 32, 33, 100):
        out.append(case(f"window-{w}", S, S, 64, True, H=4, window=w))
    out.append(case("window-33-d256", S, S, 256, True, H=4, window=33))
    out.append(case("window-32-offset-d128", 100, S, 128, True, H=4, window=32))
    out.append(case("alibi-gqa-kvlen-d128", S, S, 128, True, H=4, Hkv=2, alibi=True, kv_len=[S, 97]))
    out.append(case("alibi-gqa-d64", S, S, 64, True, H=4, Hkv=2, alibi=True))
    out.append(case("scale-1-kvlen", S, S, 64, True, scale=1.0, kv_len=[100, S]))
    return out


def tiled_cases():
    out = []
    for d in (64, 96, 128, 160):
        out.append(case(f"tiled-d{d}-causal", 384, 384, d, True, edges=tile_edge_keys(384)))
        out.append(case(f"tiled-d{d}-full", 384, 384, d, False, edges=tile_edge_keys(384)))
        out.append(case(f"tiled-gqa4-offset-d{d}", 128, 384, d, True, H=4, Hkv=1, edges=tile_edge_keys(384)))
    for d in (64, 128):
        out.append(case(f"tiled-fwd-only-288-d{d}", 256, 288, d, True, edges=tile_edge_keys(288)))
    out.append(case("tiled-d256-w8-causal", 512, 512, 256, True, edges=tile_edge_keys(512)))
    out.append(case("tiled-d256-w8-full", 512, 512, 256, False, edges=tile_edge_keys(512)))
    out.append(case("tiled-d256-384", 384, 384, 256, True, edges=tile_edge_keys(384)))
    out.append(case("tiled-d256-gqa2", 256, 256, 256, True, H=2, Hkv=1, edges=tile_edge_keys(256)))
    return out


def hot_key_inputs(seed, B, S, H, D, row, key, excess_log2, scale):
    """test_attention_tiled_overflow_fixup's pattern: small random q, k and one key past tile 0 whose
    score for query ``row`` exceeds that row's best tile-0 score by ``excess_log2`` (in log2 units; up
    to the bf16 rounding of the planted K row). Returns (q, k, v) bf16 [B, S, H, D]."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, S, H, D, generator=g) * 0.3).bfloat16()
    k = torch.randn(B, S, H, D, generator=g) * 0.3
    v = torch.randn(B, S, H, D, generator=g)
    qr = q[:, row].double()                                          # [B, H, D]
    m0 = scale * torch.einsum("bhd,bkhd->bhk", qr, k[:, :32].bfloat16().double()).amax(-1)
    alpha = (m0 + excess_log2 / LOG2E) / (scale * (qr * qr).sum(-1))
    k[:, key] = (alpha[..., None] * qr).float()
    return q, k.bfloat16(), v.bfloat16()
