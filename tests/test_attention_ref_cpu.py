"""The float64 attention oracle of tests/attention_ref.py against independent implementations, a CPU
emulation of the kernels' arithmetic against every per-element bound, and the sensitivity condition
that keeps tests/test_attention_elem_gpu.py from hiding a failure: every edge under test carries
planted pairs whose loss moves the outputs by at least 16 bounds. No GPU.

Sensitivity, as asserted below: EVERY planted pair (i, j) that the mask attends, taken out alone, moves
o (row i), dv and dk (key j) and dq (row i) by at least 16 bounds at some element. Two exceptions, both
stated in the test: a row that attends to a single key has p = 1 and no gradient, so only o is asked of
it; and at d_real = 8, where |v_j|^2 is 8 and one pair's dS cannot dominate the 160 other rows in dk's
bound, dk is asked 16 bounds of 49 pairs in 50 and 4 bounds of every pair (a kernel within its bound
that drops such a pair is still at least 3 bounds out). The generator is what makes this hold
(attention_ref.make_inputs: per-row gain on a normalised q, v_j planted into do_i with alternating
signs, unplanted rows damped). `uniform` inputs do not meet the condition at S >= 256
(test_uniform_is_not_an_edge_detector), which is why they only exercise rounding.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd.ops.attention import attention_reference

from . import attention_ref as R

ALL_CASES = R.generic_cases() + R.mask_cases() + R.tiled_cases()
IDS = [c["name"] for c in ALL_CASES]


def _ratio(actual, expected, bound):
    a = actual.double()
    fin = torch.isfinite(expected)
    err = torch.where(fin, (a - expected).abs(), torch.where(a == expected, 0.0, math.inf).double())
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("causal", [False, True])
def test_oracle_matches_sdpa_fp64(causal):
    g = torch.Generator().manual_seed(1)
    B, S, H, D = 2, 45, 3, 16
    q, k, v, do = (torch.randn(B, S, H, D, generator=g, dtype=torch.float64) for _ in range(4))
    qs, ks, vs = (t.permute(0, 2, 1, 3).clone().requires_grad_() for t in (q, k, v))
    o = F.scaled_dot_product_attention(qs, ks, vs, is_causal=causal, scale=0.3)
    gq, gk, gv = torch.autograd.grad(o, (qs, ks, vs), do.permute(0, 2, 1, 3))
    f = R.fwd(q, k, v, causal, 0.3)
    b = R.bwd(q, k, v, f["o"], f["lse"], do, causal, 0.3)
    assert torch.allclose(f["o"], o.permute(0, 2, 1, 3), rtol=0, atol=1e-12)
    assert torch.allclose(f["lse"], torch.logsumexp(
        (0.3 * qs @ ks.transpose(-1, -2)).masked_fill(~f["attend"], -math.inf), -1).detach(), rtol=0, atol=1e-12)
    for name, got, ref in (("dq", b["dq"], gq), ("dk", b["dk"], gk), ("dv", b["dv"], gv)):
        assert torch.allclose(got, ref.permute(0, 2, 1, 3), rtol=0, atol=1e-12), name


REF_CASES = [
    R.case("pin-causal", 40, 40, 16, True, kind="uniform"),
    R.case("pin-offset", 17, 40, 16, True, kind="uniform"),
    R.case("pin-gqa", 40, 40, 16, True, H=4, Hkv=2, kind="uniform"),
    R.case("pin-lengths", 40, 40, 16, False, kv_len=[40, 13], kind="uniform"),
    R.case("pin-holes", 40, 40, 16, True, holes=[(5, 6), (31, 32)], kind="uniform"),
    R.case("pin-alibi", 40, 40, 16, True, H=4, alibi=True, kind="uniform"),
    R.case("pin-window", 40, 40, 16, True, window=7, kind="uniform"),
    R.case("pin-window-offset", 17, 40, 16, True, window=7, kind="uniform"),
]


@pytest.mark.parametrize("c", REF_CASES, ids=[c["name"] for c in REF_CASES])
def test_oracle_matches_attention_reference(c):
    """Forward and, through autograd, backward of ops.attention_reference in fp32; rows that attend to
    no key are left out (the reference leaves NaN-derived zeros and lse = -inf there, the kernels
    write o = 0 and lse = +inf)."""
    m = R.materialize(c)
    qr, kr, vr = (m[n].float().requires_grad_() for n in ("q", "k", "v"))
    mask = m["key_mask"] if m["key_mask"] is not None else (m["kv_len"].long() if m["kv_len"] is not None else None)
    o, lse = attention_reference(qr, kr, vr, c["causal"], m["scale"], mask, m["alibi"], c["window"])
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    rows = f["attend"].any(-1)                                  # [B, H, Sq]
    assert rows.all() or c["name"] in ("pin-lengths", "pin-holes")
    rows_o = rows.permute(0, 2, 1)
    assert torch.allclose(o.double()[rows_o], f["o"][rows_o], rtol=0, atol=2e-5)
    assert torch.allclose(lse.double()[rows], f["lse"][rows], rtol=0, atol=2e-5)
    do = m["do"].float() * rows_o[..., None]
    gq, gk, gv = torch.autograd.grad(o, (qr, kr, vr), do)
    b = R.bwd(m["q"], m["k"], m["v"], f["o"], f["lse"], do, **m["kw"])
    for name, got, ref in (("dq", b["dq"], gq), ("dk", b["dk"], gk), ("dv", b["dv"], gv)):
        assert torch.allclose(got, ref.double(), rtol=0, atol=1e-4), (name, float((got - ref).abs().max()))


def test_empty_rows_and_excluded_keys_are_exact_zeros():
    c = R.case("pin-empty", 20, 13, 16, True, holes=[(0,), (3,)])  # causal, Sk < Sq, a hole at key 0
    m = R.materialize(c)
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    empty = ~f["attend"].any(-1)
    assert empty[:, :, :7].all() and empty[0, :, 7].all() and not empty[1, :, 7].any()
    assert (f["lse"][empty] == math.inf).all() and (f["o"].permute(0, 2, 1, 3)[empty] == 0).all()
    assert (f["bound_o"].permute(0, 2, 1, 3)[empty] == 0).all()
    b = R.bwd(m["q"], m["k"], m["v"], f["o"].bfloat16(), f["lse"].float(), m["do"], **m["kw"])
    assert (b["dq"].permute(0, 2, 1, 3)[empty] == 0).all() and (b["bound_dq"].permute(0, 2, 1, 3)[empty] == 0).all()
    for n in ("dk", "dv", "bound_dk", "bound_dv"):
        assert (b[n][m["excluded"]] == 0).all(), n
    assert all(torch.isfinite(b[n]).all() for n in ("dq", "dk", "dv"))


# ------------------------------------------------------------------------------------ emulation within bounds
_DONE = {}  # (case name, kind) -> (m, f, emulation): the sensitivity test reuses the peaked runs


def _run(c):
    key = (c["name"], c["kind"])
    if key not in _DONE:
        m = R.materialize(c)
        f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
        _DONE[key] = (m, f, _emulate(m, f))
    return _DONE[key]


def _emulate(m, f):
    oe, le = R.emulate_fwd(m["q"], m["k"], m["v"], m["scale"], f["attend"], m["alibi"])
    b = R.bwd(m["q"], m["k"], m["v"], oe, le, m["do"], **m["kw"])
    dq, dk, dv = R.emulate_bwd(m["q"], m["k"], m["v"], oe, le, m["do"], m["scale"], f["attend"], m["alibi"])
    return oe, le, b, dq, dk, dv


# uniform inputs: one head dim per kernel family is enough on the CPU
EMU = [(c, "peaked") for c in ALL_CASES] + [
    (c, "uniform") for c in ALL_CASES
    if not (c["name"].startswith(("tiled-", "generic-d")) and c["D"] not in (64, 256))]


@pytest.mark.parametrize("c,kind", EMU, ids=[f"{c['name']}-{kind}" for c, kind in EMU])
def test_emulation_meets_every_bound(c, kind):
    """fp32 scores, exp2, P and dS rounded to bf16, fp32 accumulation, bf16 results: a correct
    implementation of the kernels' arithmetic stays inside every bound, for every generator (poison
    included: every case with a per-key mask is poisoned) and mask kind."""
    m, f, (oe, le, b, dq, dk, dv) = _run(dict(c, kind=kind))
    got = {"o": _ratio(oe, f["o"], f["bound_o"]), "lse": _ratio(le, f["lse"], f["bound_lse"]),
           "dq": _ratio(dq, b["dq"], b["bound_dq"]), "dk": _ratio(dk, b["dk"], b["bound_dk"]),
           "dv": _ratio(dv, b["dv"], b["bound_dv"])}
    assert all(r <= 1.0 for r in got.values()), got
    if m["excluded"] is not None:
        assert (dk[m["excluded"]] == 0).all() and (dv[m["excluded"]] == 0).all()


# ------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("c", ALL_CASES, ids=IDS)
def test_planted_pairs_are_sixteen_bounds_tall(c):
    m, f, (oe, le, b, _, _, _) = _run(c)
    h, i, j = (torch.tensor(x) for x in zip(*m["pairs"]))
    live = f["attend"][:, h, i, j]
    single = f["attend"].sum(-1)[:, h, i] < 2  # p = 1, no gradient: o only
    sens = R.pair_sensitivity(m["q"], m["k"], m["v"], m["do"], m["scale"], f, b, m["pairs"])
    assert live.any()
    worst = {}
    for n, name in enumerate(("o", "dv", "dk", "dq")):
        msk = live if name == "o" else live & ~single
        worst[name] = float(sens[n][msk].min()) if msk.any() else math.inf
    if c["D"] == 8:
        dk = sens[2][live & ~single]
        assert float((dk >= R.SENSITIVITY).double().mean()) >= 0.98 and worst["dk"] >= 4.0, worst
        worst["dk"] = math.inf
    assert all(w >= R.SENSITIVITY for w in worst.values()), worst
    # a key just outside the window, or a poisoned key, let in: the row moves by at least as much
    att = f["attend"].clone()
    rows = torch.zeros_like(att[..., 0])
    if m["outside"]:
        ho, io, jo = (torch.tensor(x) for x in zip(*m["outside"]))
        att[:, ho, io, jo] = True
        rows[:, ho, io] = True
    if m["excluded"] is not None:
        for bi in range(c["B"]):
            ex = m["excluded"][bi].nonzero()
            if ex.numel():
                att[bi, :, :, int(ex[0])] = True
                rows[bi] = True
    if rows.any():
        f2 = R.fwd(m["q"], m["k"], m["v"], **dict(m["kw"], attend=att))
        d = (f2["o"] - f["o"]).abs()
        r = torch.where(d == 0, torch.zeros_like(d), d / f["bound_o"]).amax(-1).permute(0, 2, 1)[rows]
        assert float((r >= R.SENSITIVITY).double().mean()) == 1.0, r.min()


@pytest.mark.parametrize("S", [256, 384])
def test_uniform_is_not_an_edge_detector(S):
    """With unit-normal inputs the softmax is near uniform: the diagonal pair of most rows is worth
    less than 16 bounds of o, so a tighter threshold on randn inputs would not find a mask edge."""
    c = R.case(f"uniform-{S}", S, S, 64, False, kind="uniform")
    m = R.materialize(c)
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    oe, le, b, _, _, _ = _emulate(m, f)
    sens = R.pair_sensitivity(m["q"], m["k"], m["v"], m["do"], m["scale"], f, b, m["pairs"])
    assert float((sens[0] >= R.SENSITIVITY).double().mean()) < 0.1


def test_hot_key_excess_is_what_was_asked():
    for D, ex in ((D, ex) for D in (64, 128, 256) for ex in (90.0, 110.0, 900.0)):
        scale = D ** -0.5
        q, k, v = R.hot_key_inputs(4, 1, 512, 2, D, 330, 300, ex, scale)
        s = scale * torch.einsum("bhd,bkhd->bhk", q[:, 330].double(), k.double()) * R.LOG2E
        got = s[..., 300] - s[..., :32].amax(-1)
        assert ((got - ex).abs() <= 0.01 * ex).all(), (D, ex, got)
