"""Pins tests/norm_ref.py on the CPU: the float64 oracles against F.layer_norm / F.group_norm / F.silu with
autograd (1e-12), the concat oracle against torch.cat, the bounds against correct fp32
implementations (the CPU fallbacks of ops.layer_norm / ops.group_norm, torch.native_layer_norm /
native_group_norm for the statistics, and an fp32 emulation that sums in the kernels' chunked
order), and -- the point of the harness -- against eight planted errors, each of which must leave a
bound on at least one named case.
"""
import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd import ops

from . import norm_ref as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
RECORD: dict[str, float] = {}


def _rec(name, w):
    for k, v in w.items():
        RECORD[f"{name}.{k}"] = max(RECORD.get(f"{name}.{k}", 0.0), v)


# ------------------------------------------------------------------------------------ oracles
@pytest.mark.parametrize("nres,beta,dres", [(0, True, False), (1, False, True), (2, True, True)])
def test_layernorm_oracle_matches_autograd(nres, beta, dres):
    c = R.ln_cases(7, 24, nres, beta, dres, seed=1)["uniform"]
    h64, hb = R.ln_h(c["x"], c["res"])
    h = hb if nres else c["x"]
    o = R.ln_fwd(h, c["gamma"], c["beta"])
    hd = h.double().requires_grad_()
    g = c["gamma"].double().requires_grad_()
    b = c["beta"].double().requires_grad_() if beta else None
    y = F.layer_norm(hd, (24,), g, b, R.EPS)
    hv = hd.detach()
    assert float((y.detach() - o["y"]).abs().max()) < 1e-12
    assert float((o["mean"] - hv.mean(-1)).abs().max()) < 1e-12
    assert float((o["rstd"] - (hv.var(-1, unbiased=False) + R.EPS).rsqrt()).abs().max()) < 1e-12
    y.backward(c["dy"].double())
    ob = R.ln_bwd(c["dy"], h, c["gamma"], c["dres"])
    want_dx = hd.grad + (c["dres"].double() if dres else 0.0)
    assert float((ob["dx"] - want_dx).abs().max()) < 1e-12
    assert float((ob["dgamma"] - g.grad).abs().max()) < 1e-12
    if beta:
        assert float((ob["dbeta"] - b.grad).abs().max()) < 1e-12
    if nres:  # h: one rounding of the exact sum, at most half a bf16 ulp away
        assert float(((hb.double() - h64).abs() / R.ulp_bf16(h64)).max()) <= 0.5


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
def test_groupnorm_oracle_matches_autograd(silu, with_add):
    N, C, G, P = 2, 20, 2, 15
    c = R.gn_cases(N, C, G, P, seed=2)["uniform"]
    add = torch.randn(N, C, generator=torch.Generator().manual_seed(3)) if with_add else None
    o = R.gn_fwd(c["x"], G, c["gamma"], c["beta"], silu_on=silu, add=add)
    xd = c["x"].double()
    if with_add:
        xd = xd + add.double()[:, :, None]
    xd = xd.requires_grad_()
    g, b = c["gamma"].double().requires_grad_(), c["beta"].double().requires_grad_()
    y = F.group_norm(xd, G, g, b, R.EPS)
    if silu:
        y = F.silu(y)
    assert float((y.detach() - o["y"]).abs().max()) < 1e-12
    xg = xd.detach().view(N, G, -1)
    assert float((o["mean"] - xg.mean(-1)).abs().max()) < 1e-12
    assert float((o["rstd"] - (xg.var(-1, unbiased=False) + R.EPS).rsqrt()).abs().max()) < 1e-12
    for folded in (False, True):  # the two algebraic forms agree in float64
        of = R.gn_fwd(c["x"], G, c["gamma"], c["beta"], silu_on=silu, add=add, folded=folded)
        assert float((of["y"] - o["y"]).abs().max()) < 1e-12
    if with_add:
        return
    y.backward(c["dy"].double())
    for folded in (False, True):
        ob = R.gn_bwd(c["dy"], c["x"], G, c["gamma"], c["beta"], silu_on=silu, folded=folded)
        assert float((ob["dx"] - xd.grad).abs().max()) < 1e-11
        assert float((ob["dw"] - g.grad).abs().max()) < 1e-11
        assert float((ob["db"] - b.grad).abs().max()) < 1e-11


@pytest.mark.parametrize("phase", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
def test_concat_oracle_matches_torch_cat(phase, with_add):
    g = torch.Generator().manual_seed(4)
    N, C1, C2, H, W = 2, 8, 24, 4, 6
    d1 = torch.randn(N, C1, H, W, generator=g).to(BF16)
    x2 = torch.randn(N, C2, H, W, generator=g).to(BF16)
    a1 = torch.randn(C1, generator=g) if with_add else None
    x1 = R.dense_to_phase(d1, float("nan")) if phase else d1
    if phase:
        assert R.bits_equal(R.dense_from_phase(x1, (H, W)), d1)
        assert not R.bits_equal(R.dense_from_phase(x1, (H, W), swap=True), d1)
    cat, add, raw = R.cat_inputs(x1, x2, a1, (H, W) if phase else None)
    ref = torch.cat([d1, x2], 1).reshape(N, C1 + C2, -1)
    assert R.bits_equal(cat, ref)
    gamma, beta = R._params(C1 + C2, g)
    o = R.gn_fwd(cat, 2, gamma, beta, silu_on=True, add=add)
    full = ref.double()
    if with_add:
        full[:, :C1] += a1.double()[None, :, None]
        assert R.bits_equal(raw, full.to(BF16))
    else:
        assert R.bits_equal(raw, ref)
    want = R.gn_fwd(full, 2, gamma, beta, silu_on=True)
    assert float((o["y"] - want["y"]).abs().max()) < 1e-12


def test_case_geometry_is_what_the_names_say():
    for (N, C, G, H, W), want in R.NCHW_SHAPES:
        R.assert_geometry(R.nchw_geometry(N, C, H * W, G), want, (N, C, G, H, W))
    for (N, C, G, H, W), want in R.NHWC_SHAPES:
        R.assert_geometry(R.nhwc_geometry(N, C, H * W, G), want, (N, C, G, H, W))
    g = R.nchw_geometry(1, 10, 27 * 152, 2)
    assert g["Lg"] - g["SL"] == 10256 and 2 * 4104 < g["SL"] < 3 * 4104  # uneven last slice, boundary inside plane 2
    assert R.nchw_geometry(1, 266, 64, 2)["cpg"] == 133 and 266 % 4 == 2
    assert [R.ln_nv(d) for d in (8, 2048, 2056, 16384)] == [1, 1, 2, 8]
    assert R.ln_parts(4099) == 1024 and 4099 - 4096 == 3 and R.ln_parts(1023) == 1023


# ------------------------------------------------------------------------------------ fallbacks through the bounds
@pytest.mark.parametrize("rows,d,nres", [(5, 8, 0), (9, 2056, 1), (67, 520, 0)])
def test_layernorm_fallback_meets_every_bound(rows, d, nres):
    for kind, c in R.ln_cases(rows, d, nres, True, False, seed=5).items():
        x = c["x"].clone().requires_grad_()
        w, b = c["gamma"].clone().requires_grad_(), c["beta"].clone().requires_grad_()
        out = ops.layer_norm(x, w, b, R.EPS, residual=tuple(c["res"]))
        y, h = out if nres else (out, None)
        hh = h.detach() if nres else c["x"]
        _, mean, rstd = torch.native_layer_norm(hh.float(), (d,), w.detach().float(), b.detach().float(), R.EPS)
        got = {"h": h, "y": y, "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}
        _rec("fallback.ln", R.check_ln_fwd(f"cpu.ln.{kind}", c, got))
        y.backward(c["dy"])
        got = {"dx": x.grad, "dgamma": w.grad, "dbeta": b.grad}
        _rec("fallback.ln", R.check_ln_bwd(f"cpu.ln.{kind}", c, hh, got, R.ln_narrow(d), 0))


@pytest.mark.parametrize("shape,silu", [((2, 40, 4, 35), True), ((1, 10, 2, 4104), False), ((3, 6, 6, 2209), True)])
def test_groupnorm_fallback_meets_every_bound(shape, silu):
    N, C, G, P = shape
    for kind, c in R.gn_cases(N, C, G, P, seed=6).items():
        x = c["x"].clone().requires_grad_()
        w, b = c["gamma"].clone().requires_grad_(), c["beta"].clone().requires_grad_()
        y = ops.group_norm(x, G, w, b, R.EPS, silu=silu)
        _, mean, rstd = torch.native_group_norm(c["x"].float(), w.detach().float(), b.detach().float(), N, C, P, G, R.EPS)
        geo = R.nchw_geometry(N, C, P, G)
        _rec("fallback.gn", R.check_gn_fwd(f"cpu.gn.{kind}", c, {"y": y, "mean": mean, "rstd": rstd}, silu,
                                           R.nchw_stat_chain(geo)))
        y.backward(c["dy"])
        k = R.nchw_chain(N, P, geo["bwd"])
        _rec("fallback.gn", R.check_gn_bwd(f"cpu.gn.{kind}", c, {"dx": x.grad, "dw": w.grad, "db": b.grad}, silu, k,
                                           R.nchw_stat_chain(geo), False))


@pytest.mark.parametrize("fam", ["layer", "group", "group-nhwc"])
def test_fallback_accepts_fp32_parameters_with_bf16_activations(fam):
    g = torch.Generator().manual_seed(7)
    if fam == "layer":
        x = torch.randn(5, 16, generator=g).to(BF16).requires_grad_()
        w, b = torch.randn(16, generator=g).requires_grad_(), torch.randn(16, generator=g).requires_grad_()
        y = ops.layer_norm(x, w, b)
        ref = F.layer_norm(x.detach().float(), (16,), w.detach(), b.detach(), 1e-5)
    else:
        x = torch.randn(2, 16, 3, 5, generator=g).to(BF16)
        if fam == "group-nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_()
        w, b = torch.randn(16, generator=g).requires_grad_(), torch.randn(16, generator=g).requires_grad_()
        y = ops.group_norm(x, 4, w, b, silu=True)
        ref = F.silu(F.group_norm(x.detach().float(), 4, w.detach(), b.detach(), 1e-5))
    assert y.dtype == BF16 and R.bits_equal(y.detach().contiguous(), ref.to(BF16).contiguous())
    y.backward(torch.ones_like(y))
    assert w.grad.dtype == F32 and b.grad.dtype == F32 and x.grad.dtype == BF16


# ------------------------------------------------------------------------------------ fp32 emulations in the kernels' order
def _sum8(v):
    """Row sums in the kernels' order: 8-element vectors first, then the vectors."""
    return v.reshape(*v.shape[:-1], -1, 8).sum(-1).sum(-1)


def _ln_emul(c, h, mut=None):
    """fp32 LayerNorm forward and backward with vector-wise sums and row-chunked dgamma / dbeta,
    outputs rounded once to what the kernel stores. mut: mean-skips-last | divisor | no-m1."""
    hb, d = h.float(), h.shape[-1]
    g, dy = c["gamma"].float(), c["dy"].float()
    s = _sum8(hb) - (hb[:, -1] if mut == "mean-skips-last" else 0.0)
    mean = s / d
    cen = hb - mean[:, None]
    rstd = (_sum8(cen * cen) / (d - 1 if mut == "divisor" else d) + R.EPS).rsqrt()
    y = cen * rstd[:, None] * g + (c["beta"].float() if c["beta"] is not None else 0.0)
    xh = cen * rstd[:, None]
    gy = dy * g
    m1 = torch.zeros_like(mean) if mut == "no-m1" else _sum8(gy) / d
    m2 = _sum8(gy * xh) / d
    dx = rstd[:, None] * (gy - m1[:, None] - xh * m2[:, None])
    if c["dres"] is not None:
        dx = dx + c["dres"].float()
    chunks = torch.arange(h.shape[0]) % 4
    dg = sum((dy * xh)[chunks == i].sum(0) for i in range(4))
    db = sum(dy[chunks == i].sum(0) for i in range(4))
    return ({"h": h if c["res"] else None, "y": y.to(BF16), "mean": mean, "rstd": rstd},
            {"dx": dx.to(BF16), "dgamma": dg.to(BF16), "dbeta": db.to(BF16) if c["beta"] is not None else None})


def _ln_ratios(rows, d, nres, dres, mut, beta=True):
    out = {}
    for kind, c in R.ln_cases(rows, d, nres, beta, dres, seed=8).items():
        h = R.ln_h(c["x"], c["res"])[1] if nres else c["x"]
        f, b = _ln_emul(c, h, mut)
        w = R.check_ln_fwd(f"emul.ln.{kind}", c, f, check=False)
        w.update(R.check_ln_bwd(f"emul.ln.{kind}", c, h, b, R.ln_narrow(d), 0, check=False))
        out[kind] = w
    return out


def _gn_emul(c, layout, silu, add=None, mut=None, x=None):
    """fp32 GroupNorm with the statistics merged from slice (NCHW) or (chunk, channel) partials as
    the kernels do, the folded apply, and the backward; outputs rounded once."""
    N, C, G, P = c["N"], c["C"], c["G"], c["P"]
    xin = c["x"] if x is None else x
    if layout == "nchw":
        geo = R.nchw_geometry(N, C, P, G)
        stats = R.stats_sliced(xin, G, geo["SL"], mut=mut)
    else:
        stats = R.stats_chunked(xin, G, R.nhwc_geometry(N, C, P, G)["CH"], add=add, mut=mut)
    f = R.gn_fwd(xin, G, c["gamma"], c["beta"], silu_on=silu, add=add, dt=F32, folded=True, stats=stats)
    gmap = (torch.arange(C) // 8 * 8) // (C // G) if mut == "vector-group" else None
    b = R.gn_bwd(c["dy"], c["x"], G, c["gamma"], c["beta"], silu_on=silu, dt=F32, folded=layout == "nhwc", gmap=gmap)
    return ({"y": f["y"].to(BF16), "mean": f["mean"], "rstd": f["rstd"]},
            {"dx": b["dx"].to(BF16), "dw": b["dw"].to(BF16), "db": b["db"].to(BF16)})


def _gn_ratios(shape, layout, silu, mut, with_add=False):
    N, C, G, P = shape
    if layout == "nhwc":
        geo = R.nhwc_geometry(N, C, P, G)
        ks, k, last = R.nhwc_stat_chain(geo), R.nhwc_chain(N, P, C, G), (geo["nchunks"] - 1) * geo["CH"]
    else:
        geo = R.nchw_geometry(N, C, P, G)
        ks, k, last = R.nchw_stat_chain(geo), R.nchw_chain(N, P, geo["bwd"]), None
    out = {}
    for kind, c in R.gn_cases(N, C, G, P, last_chunk=last, seed=9).items():
        add = 3.0 * torch.randn(N, C, generator=torch.Generator().manual_seed(10)) if with_add else None
        f, b = _gn_emul(c, layout, silu, add, mut)
        w = R.check_gn_fwd(f"emul.gn.{kind}", c, f, silu, ks, add=add, check=False)
        if not with_add:
            w.update(R.check_gn_bwd(f"emul.gn.{kind}", c, b, silu, k, ks, layout == "nhwc", check=False))
        out[kind] = w
    return out


def _cat_ratios(swap):
    g = torch.Generator().manual_seed(11)
    N, C1, C2, H, W, G = 1, 8, 24, 4, 6, 2
    out = {}
    for kind, c in R.gn_cases(N, C1 + C2, G, H * W, seed=12).items():
        x1 = R.dense_to_phase(c["x"][:, :C1].reshape(N, C1, H, W), 0.0)
        x2 = c["x"][:, C1:].reshape(N, C2, H, W)
        cat_ok, add, _ = R.cat_inputs(x1, x2, torch.randn(C1, generator=g), (H, W))
        cat, _, _ = R.cat_inputs(x1, x2, None, (H, W), swap=swap)
        f, _ = _gn_emul(c, "nhwc", True, add, x=cat)
        ks = R.nhwc_stat_chain(R.nhwc_geometry(N, C1 + C2, H * W, G))
        out[kind] = R.check_gn_fwd(f"emul.cat.{kind}", c, f, True, ks, add=add, x64=cat_ok, check=False)
    return out


def _worst(r):
    return max(max(w.values()) for w in r.values())


LN_EMUL = [(5, 8, 0, False), (9, 2056, 2, True), (67, 520, 1, True), (3, 16384, 0, False)]
GN_EMUL = [((2, 40, 4, 35), "nhwc", True), ((1, 80, 8, 65), "nhwc", False), ((1, 16, 2, 4097), "nhwc", True),
           ((1, 10, 2, 4104), "nchw", True), ((1, 4, 1, 4225), "nchw", False), ((2, 20, 2, 36), "nchw", True)]


def test_fp32_emulations_meet_every_bound():
    """An fp32 implementation that sums in another order than the one the bounds were taken from --
    vector-wise rows, slice and chunk partials merged with Chan's formula, the folded apply -- stays
    under every bound on every named case."""
    for rows, d, nres, dres in LN_EMUL:
        r = _ln_ratios(rows, d, nres, dres, None)
        RECORD[f"emul.ln.{rows}x{d}"] = _worst(r)
        assert _worst(r) <= 1.0, (rows, d, r)
    for shape, layout, silu in GN_EMUL:
        for with_add in ((False, True) if layout == "nhwc" else (False,)):
            r = _gn_ratios(shape, layout, silu, None, with_add)
            RECORD[f"emul.gn.{layout}.{shape}{'+add' if with_add else ''}"] = _worst(r)
            assert _worst(r) <= 1.0, (shape, layout, r)
    r = _cat_ratios(False)
    RECORD["emul.cat"] = _worst(r)
    assert _worst(r) <= 1.0, r


def _bites(name, ratios, outputs):
    """The planted error leaves a bound of one of ``outputs`` on at least one named case."""
    hit = {k: {o: w[o] for o in outputs if o in w} for k, w in ratios.items()}
    worst = max(max(h.values()) for h in hit.values())
    RECORD[f"planted.{name}"] = worst
    print(f"[norm] planted {name}: " + ", ".join(f"{k} {max(h.values()):.3g}" for k, h in hit.items()))
    assert worst > 1.0, (name, hit)
    return hit


def test_planted_last_element_left_out_of_the_mean():
    _bites("mean-skips-last", _ln_ratios(9, 2056, 0, False, "mean-skips-last"), ("mean", "y"))


def test_planted_divisor_off_by_one_is_caught_by_rstd_alone():
    """d - 1 under the variance moves rstd by 1 / (2d) relative: 2.4e-4 at d = 2056, a sixteenth of a
    bf16 rounding, and 3e-5 at d = 16384. The fp32 check of rstd is off by 247 and 12.7 bounds on every
    case with a variance; y (without beta: with it, an element whose xhat gamma cancels beta is a y
    near 0 that shows more) reaches 1.05 bounds at most, a rounding that happened to fall the other
    way, and at d = 16384 dgamma and the unplanted dx stay inside theirs."""
    for rows, d in ((9, 2056), (3, 16384)):
        r = _ln_ratios(rows, d, 0, False, "divisor", beta=False)
        hit = _bites(f"divisor.{d}", r, ("rstd",))
        assert min(h["rstd"] for k, h in hit.items() if k != "constant") > 10.0
        assert max(w["y"] for w in r.values()) < 1.1  # the bf16 output alone all but lets it through
        RECORD[f"planted.divisor.{d}.y"] = max(w["y"] for w in r.values())


def test_planted_m1_dropped_in_the_backward():
    _bites("no-m1", _ln_ratios(67, 520, 1, True, "no-m1"), ("dx",))


def test_planted_wrong_slice_count_in_the_merge():
    hit = _bites("slice-count", _gn_ratios((1, 10, 2, 4104), "nchw", True, "slice-count"), ("mean", "rstd", "y"))
    assert hit["offset-channel"]["rstd"] > 1.0


def test_planted_group_index_per_vector_at_cg_10():
    _bites("vector-group", _gn_ratios((2, 40, 4, 35), "nhwc", True, "vector-group"), ("dx", "dw"))


def test_planted_last_chunk_counted_as_a_full_one():
    _bites("chunk-count", _gn_ratios((1, 80, 8, 65), "nhwc", False, "chunk-count"), ("mean", "rstd", "y"))
    _bites("chunk-count-4097", _gn_ratios((1, 16, 2, 4097), "nhwc", True, "chunk-count"), ("mean", "rstd"))


def test_planted_add_left_out_of_the_statistics():
    _bites("no-add", _gn_ratios((2, 40, 4, 35), "nhwc", True, "no-add", with_add=True), ("mean", "rstd", "y"))


def test_planted_phases_swapped():
    _bites("phase-swap", _cat_ratios(True), ("mean", "rstd", "y"))


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n    worst error/bound per check (CPU):")
    for k in sorted(RECORD):
        print(f"    {k:<44s}{RECORD[k]:.3g}")
