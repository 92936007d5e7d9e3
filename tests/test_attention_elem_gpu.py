"""The flash-attention kernels (csrc/kernels/attention.hip, attention_tiled.hip), forward and backward,
per element against the float64 oracle of tests/attention_ref.py (pinned on the CPU by
tests/test_attention_ref_cpu.py), on inputs that put the softmax weight on the (query, key) pairs at
the edges under test and that poison every key a mask excludes.

Each case calls ops.attention._fwd and _bwd directly on strided views of guard-banded buffers: o, dq,
dk and dv have a head stride 8 elements wider than d_real, the columns between and the 64-element
bands on either side hold a NaN sentinel and must be intact afterwards; lse sits between bands too.
The kernels that ran are read from torch.profiler, so each case tests the instantiation it names.
The backward oracle takes the o and lse the forward kernel stored, so forward error stays out of the
backward bounds; every backward runs twice and must repeat bit for bit. Excluded keys have dk = dv = 0
exactly, rows without a key o = 0, lse = +inf and dq = 0 exactly, and every output is finite.

Not covered here: the max_col variant of the narrow forward folds the scale into K and rounds the
row maximum to bf16, a different error model; it stays on tests/test_attention_masks_gpu.py. The
rowsum variants take the softmax denominator from bf16-rounded probabilities, so their lse (which
inference never reads) is outside bound_lse and is not compared.

Worst error/bound ratio observed per check on an MI355X (1.0 is the bound; printed by every run as
"[attention] <name>: worst error/bound ..."):

    check              o       lse     dq      dk      dv
    generic            0.872   0.019   0.868   0.935   0.964
    mask               0.822   0.021   0.869   0.898   0.845
    fused              0.767   0.011   0.724   0.851   0.835
    tiled              0.880   0.015   0.894   0.937   0.923
    narrow             0.777   0.013   0.723   0.779   0.693
    wide               0.933   -       -       -       -
    rescale-free-90    0.887   0.014   -       -       -
    rescale-free-110   0.900   0.007   -       -       -
    rescale-free-900   0.632   0.009   -       -       -

(A module fixture prints this table after the tests.) The ratios near 0.9 are bf16 rounding itself, as the CPU
emulation shows (0.6 to 0.96 on the same inputs, tests/test_attention_ref_cpu.py). No kernel missed
a bound.
"""
import re

import pytest
import torch

from kubernetes_cloud_amd.ops import _lib
from kubernetes_cloud_amd.ops import attention as A

from . import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
PAD = 8  # extra elements per head row of every output buffer


def _pick_d(d):
    return next(D for D in (64, 96, 128, 160, 256) if d <= D)


class Out:
    """[B, S, H, d] output view with head stride d + pad inside a Guarded buffer whose payload starts
    out as the sentinel everywhere."""

    def __init__(self, B, S, H, d, pad=PAD):
        self.shape, self.pad = (B, S, H, d + pad), pad
        self.g = R.Guarded(B * S * H * (d + pad), BF16, DEV)
        self.g.v.view(torch.int16).fill_(self.g.pat)
        self.full = self.g.v.view(B, S, H, d + pad)
        self.v = self.full[..., :d]

    def check(self, what):
        assert self.g.intact(), f"{what}: guard band overwritten"
        if self.pad:
            between = self.full[..., self.shape[3] - self.pad:].contiguous().view(torch.int16).cpu()
            assert bool((between == self.g.pat).all()), f"{what}: columns past d_real overwritten"


def _lse_buf(B, H, Sq):
    g = R.Guarded(B * H * Sq, torch.float32, DEV)
    g.v.view(torch.int32).fill_(g.pat)
    return g, g.v.view(B, H, Sq)


def _ran(names, base, D=None):
    pat = re.compile(rf"\b{base}<\s*{D}\s*[,>]" if D is not None else rf"\b{base}\b")
    return any(pat.search(n) for n in names)


def _assert_kernels(names, expect, absent):
    uniq = sorted(set(n for n in names if "attn" in n))
    for base, D in expect:
        assert _ran(names, base, D), (f"{base}<{D}> did not run", uniq)
    for base in absent:
        assert not any(base in n for n in uniq), (f"{base} ran", uniq)


def _dev_mask(m):
    if m["key_mask"] is not None:
        return A.native_mask(m["key_mask"], DEV)
    return A.native_mask(m["kv_len"], DEV) if m["kv_len"] is not None else None


def _check_fwd(fam, m, f, o, lse, check_lse=True):
    R.assert_within(f"attn.{fam}.o", o, f["o"], f["bound_o"])
    if check_lse:
        R.assert_within(f"attn.{fam}.lse", lse, f["lse"], f["bound_lse"])
    assert torch.isfinite(o.float()).all()


def _check_bwd(fam, m, b, dq, dk, dv):
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t.float()).all(), n
        R.assert_within(f"attn.{fam}.{n}", t, b[n], b[f"bound_{n}"])
    if m["excluded"] is not None and m["excluded"].any():  # the bounds are 0 there; this is the plain statement
        ex = m["excluded"].to(DEV)
        assert float(dk[ex].float().abs().max()) == 0.0 and float(dv[ex].float().abs().max()) == 0.0


def run_case(c, fam, fwd_kernels, bwd_kernels, absent=(), backward=True, fused=False, mf=None):
    """One case end to end; returns nothing, asserts everything the module docstring lists."""
    m = mf[0] if mf else R.materialize(c)
    B, Sq, Sk, H, Hkv, d = (c[n] for n in ("B", "Sq", "Sk", "H", "Hkv", "D"))
    f = mf[1] if mf else R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    if fused:  # one [B, S, 3, H, d] buffer, as the fused QKV GEMM leaves it
        assert Sq == Sk and H == Hkv
        gin = R.Guarded(B * Sq * 3 * H * d, BF16, DEV, torch.stack([m["q"], m["k"], m["v"]], 2).reshape(-1))
        v5 = gin.v.view(B, Sq, 3, H, d)
        q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
        before = gin.buf.clone()
    else:
        q, k, v = (m[n].to(DEV) for n in ("q", "k", "v"))
    do = m["do"].to(DEV)
    alibi = m["alibi"].to(DEV, torch.float32).contiguous() if m["alibi"] is not None else None
    mask = _dev_mask(m)
    o = Out(B, Sq, H, d)
    glse, lse = _lse_buf(B, H, Sq)
    if fused:
        gd = R.Guarded(B * Sq * 3 * H * d, BF16, DEV)
        gd.v.view(torch.int16).fill_(gd.pat)
        outs = [gd, gd]
    else:
        outs = [(Out(B, Sq, H, d), Out(B, Sk, Hkv, d), Out(B, Sk, Hkv, d)) for _ in range(2)]

    def grads(i):
        if fused:
            d5 = gd.v.view(B, Sq, 3, H, d)
            return d5[:, :, 0], d5[:, :, 1], d5[:, :, 2]
        return tuple(t.v for t in outs[i])

    torch.cuda.synchronize()  # the copies and fills above stay out of the profile
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        A._fwd(q, k, v, c["causal"], m["scale"], mask, alibi, out=o.v, window=c["window"], lse=lse)
        torch.cuda.synchronize()
        if backward:
            A._bwd(q, k, v, o.v, do, lse, *grads(0), c["causal"], m["scale"], mask, alibi, c["window"])
            torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    _assert_kernels(names, list(fwd_kernels) + (list(bwd_kernels) if backward else []), absent)

    _check_fwd(fam, m, f, o.v, lse)
    o.check("o")
    assert glse.intact(), "lse: guard band overwritten"
    if fused:
        assert R.bits_equal(gin.buf, before), "the forward wrote to the fused QKV buffer"
    if not backward:
        return
    b = R.bwd(m["q"], m["k"], m["v"], o.v.cpu(), lse.cpu(), m["do"], **m["kw"])
    first = [t.clone() for t in grads(0)]
    _check_bwd(fam, m, b, *first)
    if fused:
        assert gd.intact(), "dQKV: guard band overwritten"
        assert R.bits_equal(gin.buf, before), "the backward wrote to the fused QKV buffer"
        gd.v.view(torch.int16).fill_(gd.pat)
    A._bwd(q, k, v, o.v, do, lse, *grads(1), c["causal"], m["scale"], mask, alibi, c["window"])
    torch.cuda.synchronize()
    for n, t0, t1 in zip(("dq", "dk", "dv"), first, grads(1)):
        assert R.bits_equal(t0.contiguous(), t1.contiguous()), f"{n}: two runs differ"
    if not fused:
        for pair in outs:
            for n, t in zip(("dq", "dk", "dv"), pair):
                t.check(n)


def _generic_kernels(d):
    D = _pick_d(d)
    dq = "attn_bwd_dq32_kernel" if D == 256 else "attn_bwd_dq_kernel"
    return [("attn_fwd_kernel", D)], [("attn_bwd_dkdv_kernel", D), (dq, D)]


GENERIC = R.generic_cases()
MASKS = R.mask_cases()
TILED = R.tiled_cases()


# ------------------------------------------------------------------------------------ generic kernels
@pytest.mark.parametrize("c", GENERIC, ids=[c["name"] for c in GENERIC])
def test_generic(c):
    """Every compiled head dim and every padded one, causal and not, at sizes with partial blocks,
    waves and tiles, a causal offset, one query, and causal Sk < Sq (rows 0..69 without a key)."""
    fk, bk = _generic_kernels(c["D"])
    run_case(c, "generic", fk, bk, absent=("tiled", "w8"))


@pytest.mark.parametrize("c", MASKS, ids=[c["name"] for c in MASKS])
def test_mask_edges(c):
    """kv_len, holes at word boundaries and at key 0, windows, ALiBi and scale = 1 with planted pairs on
    the edge and poisoned excluded keys."""
    fk, bk = _generic_kernels(c["D"])
    run_case(c, "mask", fk, bk, absent=("tiled", "w8"))


def test_fused_qkv_buffer():
    """q, k, v are slices of one [B, S, 3, H, D] buffer and dq, dk, dv of another: the forward leaves
    the first bit-identical, the backward fills every slice of the second with its own gradient (a
    slice written through another's pointer fails that slice's bounds) and stays inside it."""
    c = R.case("fused-qkv-d64", R.S_ODD, R.S_ODD, 64, True, edges=R.tile_edge_keys(R.S_ODD))
    fk, bk = _generic_kernels(64)
    run_case(c, "fused", fk, bk, absent=("tiled", "w8"), fused=True)


# ------------------------------------------------------------------------------------ full-tile kernels
def _tiled_kernels(c):
    D, name = c["D"], c["name"]
    fwd = [("attn_fwd_tiled_kernel", D)]
    bwd = [("attn_bwd_dkdv_tiled_kernel", D), ("attn_bwd_dq_tiled_kernel", D)]
    if "fwd-only" in name:
        bwd = _generic_kernels(D)[1]
    if D == 256:
        if c["Sq"] % 256 == 0:
            fwd = [("attn_fwd_w8_kernel", 256)]
        if c["H"] == c["Hkv"]:
            bwd = [("attn_bwd_dkdv_w8_kernel", 256), ("attn_bwd_dq_tiled_kernel", 256)]
    return fwd, bwd


def _assert_no_overflow(c):
    """No row comes near the 2^100 row-sum flag of the rescale-free forward, so what is compared is
    the full-tile kernel's own output and not the generic fixup's."""
    m = R.materialize(c)
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    qd, kd, _ = R._heads(m["q"], m["k"], m["v"])
    s0 = (m["scale"] * qd @ kd[:, :, :32].transpose(-1, -2)).masked_fill(~f["attend"][..., :32], -float("inf")).amax(-1)
    assert float(((f["lse"] - s0) * R.LOG2E).max()) < 90.0
    return m, f


@pytest.mark.parametrize("c", TILED, ids=[c["name"] for c in TILED])
def test_tiled(c):
    """Three key blocks, GQA 4:1 with a causal offset of 256, Sk = 288 (full-tile forward, generic
    backward) and the three D = 256 launch variants."""
    mf = _assert_no_overflow(c)
    fk, bk = _tiled_kernels(c)
    run_case(c, "tiled", fk, bk, mf=mf)


def test_variant_0_uses_the_four_wave_d256_kernels():
    c = R.case("tiled-d256-variant0", 512, 512, 256, True, edges=R.tile_edge_keys(512))
    old = A.set_variant(0)
    try:
        run_case(c, "tiled", [("attn_fwd_tiled_kernel", 256)],
                 [("attn_bwd_dkdv_tiled_kernel", 256), ("attn_bwd_dq_tiled_kernel", 256)], absent=("w8",))
    finally:
        A.set_variant(old)


def test_tiled_path_off_uses_the_generic_kernels():
    c = R.case("tiled-off-d128", 384, 384, 128, True, edges=R.tile_edge_keys(384))
    A.set_tiled_path(False)  # returns nothing; on is the library's default and what every other test assumes
    try:
        fk, bk = _generic_kernels(128)
        run_case(c, "generic", fk, bk, absent=("tiled", "w8"))
    finally:
        A.set_tiled_path(True)


# ------------------------------------------------------------------------------------ narrow 48-wide storage
def _narrow_inputs(c, rowsum):
    m = R.materialize(c)
    pad = lambda t: torch.cat([t, torch.zeros(*t.shape[:-1], 8, dtype=t.dtype)], -1)  # noqa: E731
    for n in ("q", "k", "v", "do"):
        m[n] = pad(m[n])
    if rowsum:
        m["v"][..., 40] = 1.0
    return m


@pytest.mark.parametrize("rowsum", [False, True])
def test_narrow_48_forward(rowsum):
    """40-wide heads stored 48 wide in one fused buffer (D = 64 LDS images): payload columns within the
    bounds, pad columns exactly 0 (their bound is 0: A_o = 0 there), the row-sum column within
    bound_o of 1 (A_o = 1 there)."""
    c = R.case("narrow-48", 256, 256, 40, False, edges=R.tile_edge_keys(256))
    m = _narrow_inputs(c, rowsum)
    B, S, H = c["B"], c["Sq"], c["H"]
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    gin = R.Guarded(B * S * 3 * H * 48, BF16, DEV, torch.stack([m["q"], m["k"], m["v"]], 2).reshape(-1))
    v5 = gin.v.view(B, S, 3, H, 48)
    before = gin.buf.clone()
    o = Out(B, S, H, 48)
    glse, lse = _lse_buf(B, H, S)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        A._fwd(v5[:, :, 0], v5[:, :, 1], v5[:, :, 2], False, m["scale"], None, None, out=o.v,
               rowsum_col=40 if rowsum else -1, lse=lse)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    want = r"attn_fwd_tiled_kernel<\s*64,.*\b40,\s*48" if rowsum else r"attn_fwd_tiled_kernel<\s*64,.*-1,\s*48"
    assert any(re.search(want, n) for n in names), sorted(set(names))
    _check_fwd("narrow", m, f, o.v, lse, check_lse=not rowsum)
    if rowsum:
        assert float((f["o"][..., 40] - 1).abs().max()) < 1e-12 and float(f["A_o"][..., 41:].abs().max()) == 0.0
    else:
        assert float(o.v[..., 40:].float().abs().max()) == 0.0
    o.check("o")
    assert glse.intact() and R.bits_equal(gin.buf, before)


def test_narrow_48_backward():
    c = R.case("narrow-48-bwd", 256, 256, 40, False, edges=R.tile_edge_keys(256))
    m = _narrow_inputs(c, False)
    B, S, H = c["B"], c["Sq"], c["H"]
    gin = R.Guarded(B * S * 3 * H * 48, BF16, DEV, torch.stack([m["q"], m["k"], m["v"]], 2).reshape(-1))
    v5 = gin.v.view(B, S, 3, H, 48)
    q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
    before = gin.buf.clone()
    do = m["do"].to(DEV)
    o, lse = A._fwd(q, k, v, False, m["scale"], None, None)
    b = R.bwd(m["q"], m["k"], m["v"], o.cpu(), lse.cpu(), m["do"], **m["kw"])
    runs = []
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(2):
            gd = R.Guarded(B * S * 3 * H * 48, BF16, DEV)
            gd.v.view(torch.int16).fill_(gd.pat)
            d5 = gd.v.view(B, S, 3, H, 48)
            A._bwd(q, k, v, o, do, lse, d5[:, :, 0], d5[:, :, 1], d5[:, :, 2], False, m["scale"], None, None)
            torch.cuda.synchronize()
            runs.append((gd, d5))
    names = [e.name for e in prof.events()]
    for kern in ("attn_bwd_dq_tiled_kernel", "attn_bwd_dkdv_tiled_kernel"):
        assert any(re.search(rf"{kern}<\s*64,.*\b48", n) for n in names), (kern, sorted(set(names)))
    gd, d5 = runs[0]
    _check_bwd("narrow", m, b, d5[:, :, 0], d5[:, :, 1], d5[:, :, 2])
    assert float(d5[..., 40:].float().abs().max()) == 0.0
    assert gd.intact() and runs[1][0].intact() and R.bits_equal(gin.buf, before)
    assert R.bits_equal(gd.v, runs[1][0].v), "two runs differ"


# ------------------------------------------------------------------------------------ 512-wide head
def test_wide_head_512_forward():
    """kca_attn_fwd_wide (attn_fwd_w8_kernel<512, false, 4, 2>), called as ops.wide_head_attention
    calls it but with o between guard bands, at Sq = 128, Sk = 160. q is halved as the VAE's is, which
    keeps the planted score (3 * 128 / sqrt(512) = 17) far from the row-sum flag this kernel has no
    fixup for; no flag may be set."""
    B, Sq, Sk, D = 2, 128, 160, 512
    c = R.case("wide-512", Sq, Sk, D, False, H=1, edges=R.tile_edge_keys(Sk), q_gain=0.5)
    m = R.materialize(c)
    f = R.fwd(m["q"], m["k"], m["v"], **m["kw"])
    q, k, v = (m[n].to(DEV)[:, :, 0] for n in ("q", "k", "v"))
    o = Out(B, Sq, 1, D)
    flags = torch.full((4 * (Sq // 128) * B,), -1, device=DEV, dtype=torch.int32)
    st = lambda t: (t.stride(0), t.stride(1), 0)  # noqa: E731
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        rc = _lib.call_rc("kca_attn_fwd_wide", q.data_ptr(), k.data_ptr(), v.data_ptr(), o.v.data_ptr(), None,
                          *st(q), *st(k), *st(v), o.v.stride(0), o.v.stride(1), 0, B, Sq, Sk, 1, 1, D,
                          float(m["scale"]), flags.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
    assert rc == 0
    assert _ran([e.name for e in prof.events()], "attn_fwd_w8_kernel", 512)
    assert not bool(flags.any())
    _check_fwd("wide", m, f, o.v, None, check_lse=False)
    o.check("o")


# ------------------------------------------------------------------------------------ rescale-free forward
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("excess", [90.0, 110.0, 900.0])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_rescale_free_forward_and_fixup(D, excess, causal):
    """test_attention_tiled_overflow_fixup's pattern with its claim asserted: key 300 (past tile 0)
    scores `excess` log2 units above query 330's best tile-0 score -- below the 2^100 row-sum flag,
    above it, far above it. The overflow flags are read back and compared, wave by wave, with the rows
    whose row sum relative to their tile-0 maximum the oracle puts past 2^100 (a wave with a row
    within 2 log2 units of the threshold may go either way): none at 90, so every row there is the
    rescale-free kernel's own; at 110 and 900 exactly the waves that hold such a row, so the generic
    launch (which runs only flagged 128-row blocks) rewrote those blocks and no others -- with the
    causal mask rows 0..299 never see the key and blocks 0 and 1 stay unflagged. o and lse meet the
    per-element bounds on every row, kept or rewritten. Sq = 512: the 8-wave kernel's two 256-row
    blocks report their flags in the four-wave layout, reversed under the causal mask."""
    B, S, H = 1, 512, 2
    scale = D ** -0.5
    q, k, v = R.hot_key_inputs(4, B, S, H, D, 330, 300, excess, scale)
    f = R.fwd(q, k, v, causal, scale)
    o = Out(B, S, H, D)
    glse, lse = _lse_buf(B, H, S)
    nqb = S // 128
    gflags = R.Guarded(4 * nqb * B * H, torch.int32, DEV)
    gflags.v.fill_(-1)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        A._fwd(q.to(DEV), k.to(DEV), v.to(DEV), causal, scale, None, None, out=o.v, lse=lse, flags=gflags.v)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    _assert_kernels(names, [("attn_fwd_w8_kernel" if D == 256 else "attn_fwd_tiled_kernel", D),
                            ("attn_fwd_kernel", D)], ())
    # log2 of each row's sum of 2^(s - m0), m0 the row's best attended score among keys 0..31
    qd, kd, _ = R._heads(q, k, v)
    s0 = (scale * qd @ kd[:, :, :32].transpose(-1, -2)).masked_fill(~f["attend"][..., :32], -float("inf")).amax(-1)
    over = ((f["lse"] - s0) * R.LOG2E).view(B * H, nqb, 4, 32)           # [bh, block, wave, row]
    sure_set = (over > 102.0).any(-1)
    sure_clear = (over < 98.0).all(-1)
    if causal:  # flags are stored in launch order: the last block first
        sure_set, sure_clear = sure_set.flip(1), sure_clear.flip(1)
    got = gflags.v.cpu().view(B * H, nqb, 4)
    assert gflags.intact() and bool(((got == 0) | (got == 1)).all()), got
    assert bool((got[sure_set] == 1).all()) and bool((got[sure_clear] == 0).all()), (got, sure_set, sure_clear)
    if excess == 90.0:
        assert bool(sure_clear.all())
    else:
        assert bool(sure_set.any())
        if causal or excess == 110.0:  # (at 900 without the mask every wave holds a row past the threshold)
            assert bool(sure_clear.all(-1).any()), "no block is expected to stay unflagged"
    m = {"excluded": None}
    _check_fwd(f"rescale-free-{int(excess)}", m, f, o.v, lse)
    o.check("o")
    assert glse.intact()


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    """Prints, after the module's tests, the worst ratio per kernel family and output that this
    process saw (the table of the module docstring). No assertion: assert_within has made them."""
    yield
    fams = sorted({n.split(".")[1] for n in R.WORST if n.startswith("attn.")})
    print("\n    check            " + "".join(f"{n:<8s}" for n in ("o", "lse", "dq", "dk", "dv")))
    for fam in fams:
        row = [R.WORST.get(f"attn.{fam}.{n}") for n in ("o", "lse", "dq", "dk", "dv")]
        print(f"    {fam:<17s}" + "".join(f"{'-' if r is None else format(r, '.3f'):<8s}" for r in row))
