"""The emit-and-consume D = 256 attention backward, bit 2 of kca_attn_set_variant
(csrc/kernels/attention_tiled.hip): attn_bwd_dkdv_w8_kernel<.., EMIT_DS> writes each bf16 dS tile
once to a workspace and attn_bwd_dq_ds_kernel computes dQ = dS.K from it, in place of the dQ kernel
that recomputes S, dP and P.

Inputs, the float64 oracle and the bounds are tests/attention_ref.py's, with pairs planted on the
32-key tile edges: a dS tile stored or read at the wrong index moves a planted pair's weight to other
rows. Every case calls ops.attention._bwd with an explicit workspace under variant 7 and asserts the
fp64 bounds, two bit-equal runs, dK / dV / dQ bit-equal to variant 3 (the two-kernel path), and, from
torch.profiler, which kernels ran. The workspace tests show that the consumer reads only what the
producer wrote in the same call; the fallbacks show that everything outside the path is variant 3.
"""
import pytest
import torch

from kubernetes_cloud_amd import ops
from kubernetes_cloud_amd.ops import _lib
from kubernetes_cloud_amd.ops import attention as A

from . import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
D = 256
# dQ of the workspace path is bit-equal to the two-kernel path: the dS bits are the same (the S MFMA with
# A and B swapped sums the same products over the same k index) and every dQ MFMA gets the same keys
# in the same k-slots in the same tile order.
DQ_BIT_EQUAL = True

EMIT = ("attn_bwd_dkdv_w8_kernel", "attn_bwd_dq_ds_kernel")
TWO_KERNEL = ("attn_bwd_dkdv_w8_kernel", "attn_bwd_dq_tiled_kernel")


def _case(name, Sq, Sk, causal, B=1, H=1, Hkv=None, d=D):
    return R.case(name, Sq, Sk, d, causal, B=B, H=H, Hkv=Hkv, edges=R.tile_edge_keys(Sk))


CASES = [
    _case("ds-128-causal", 128, 128, True),                   # one key block: diagonal and masked-zero tiles only
    _case("ds-256-causal", 256, 256, True, H=2),
    _case("ds-256-full", 256, 256, False, H=2),
    _case("ds-384-causal", 384, 384, True, H=2),              # odd tile counts through the three buffers
    _case("ds-384-full", 384, 384, False, H=2),
    _case("ds-offset-128x384", 128, 384, True, H=2),          # bottom-right offset 256
    _case("ds-1024-causal", 1024, 1024, True),                # the long loop
]

_SETUP = {}


def _setup(c):
    """Inputs on the device, the forward kernel's o and lse, and the fp64 backward oracle: once per case."""
    if c["name"] not in _SETUP:
        m = R.materialize(c)
        q, k, v, do = (m[n].to(DEV) for n in ("q", "k", "v", "do"))
        o, lse = A._fwd(q, k, v, c["causal"], m["scale"], None, None)
        b = R.bwd(m["q"], m["k"], m["v"], o.cpu(), lse.cpu(), m["do"], **m["kw"])
        _SETUP[c["name"]] = dict(m=m, q=q, k=k, v=v, do=do, o=o, lse=lse, b=b)
    return _SETUP[c["name"]]


def _workspace(c, q, k):
    old = A.set_variant(7)
    try:
        ws = A.bwd_workspace(q, k, c["causal"])
    finally:
        A.set_variant(old)
    assert ws is not None and ws.numel() == c["B"] * c["H"] * c["Sq"] * c["Sk"] * 2
    return ws


def _run(c, s, variant, ws, q=None, k=None, v=None, grads=None):
    """One backward under `variant`; returns (dq, dk, dv), the attention kernel names that ran."""
    q, k, v = (s["q"], s["k"], s["v"]) if q is None else (q, k, v)
    if grads is None:
        grads = tuple(torch.full(t.shape, float("nan"), device=DEV, dtype=BF16) for t in (q, k, k))
    old = A.set_variant(variant)
    try:
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            A._bwd(q, k, v, s["o"], s["do"], s["lse"], *grads, c["causal"], s["m"]["scale"], None, None, ws=ws)
            torch.cuda.synchronize()
    finally:
        A.set_variant(old)
    return grads, sorted(set(e.name for e in prof.events() if "attn_bwd" in e.name and "preprocess" not in e.name))


def _assert_ran(names, expect):
    assert len(names) == 2 and all(any(e + "<" in n for n in names) for e in expect), (expect, names)


def _assert_equal(got, ref, what):
    for n, a, b in zip(("dq", "dk", "dv"), got, ref):
        if n != "dq" or DQ_BIT_EQUAL:
            assert R.bits_equal(a.contiguous(), b.contiguous()), f"{n}: {what}"


def _check_bounds(s, grads):
    for n, t in zip(("dq", "dk", "dv"), grads):
        assert torch.isfinite(t.float()).all(), n
        R.assert_within(f"attn.ds.{n}", t, s["b"][n], s["b"][f"bound_{n}"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_emit_and_consume(c):
    s = _setup(c)
    ws = _workspace(c, s["q"], s["k"])
    first, names = _run(c, s, 7, ws)
    _assert_ran(names, EMIT)
    _check_bounds(s, first)
    again, _ = _run(c, s, 7, ws)
    _assert_equal(again, first, "two runs differ")
    assert R.bits_equal(again[0], first[0]), "dq: two runs differ"
    ref, names3 = _run(c, s, 3, None)
    _assert_ran(names3, TWO_KERNEL)
    _assert_equal(first, ref, "differs from variant 3")


def test_fused_qkv_slices_between_guard_bands():
    """q/k/v and dq/dk/dv are slices of fused [B, S, 3, H, D] buffers: token stride 3 H D, the buffers'
    guard bands intact, the inputs bit-unchanged."""
    c = _case("ds-fused-256", 256, 256, True, B=2, H=3)
    s = _setup(c)
    B, S, H = 2, 256, 3
    m = s["m"]
    gin = R.Guarded(B * S * 3 * H * D, BF16, DEV, torch.stack([m["q"], m["k"], m["v"]], 2).reshape(-1))
    v5 = gin.v.view(B, S, 3, H, D)
    before = gin.buf.clone()
    ws = _workspace(c, s["q"], s["k"])
    outs = []
    for variant, w in ((7, ws), (7, ws), (3, None)):
        gd = R.Guarded(B * S * 3 * H * D, BF16, DEV)
        gd.v.view(torch.int16).fill_(gd.pat)
        d5 = gd.v.view(B, S, 3, H, D)
        g, names = _run(c, s, variant, w, v5[:, :, 0], v5[:, :, 1], v5[:, :, 2], (d5[:, :, 0], d5[:, :, 1], d5[:, :, 2]))
        _assert_ran(names, EMIT if variant == 7 else TWO_KERNEL)
        assert gd.intact(), "dQKV: guard band overwritten"
        outs.append(g)
    assert R.bits_equal(gin.buf, before), "the backward wrote to the fused QKV buffer"
    _check_bounds(s, outs[0])
    _assert_equal(outs[1], outs[0], "two runs differ")
    assert R.bits_equal(outs[1][0].contiguous(), outs[0][0].contiguous()), "dq: two runs differ"
    _assert_equal(outs[0], outs[2], "differs from variant 3")


# ------------------------------------------------------------------------------------ the workspace
WS_CASE = CASES[1]


def test_workspace_between_guard_bands():
    c, s = WS_CASE, _setup(WS_CASE)
    n = c["B"] * c["H"] * c["Sq"] * c["Sk"] * 2
    g = R.Guarded(n, torch.uint8, DEV)
    got, names = _run(c, s, 7, g.v)
    _assert_ran(names, EMIT)
    assert g.intact(), "workspace: guard band overwritten"
    _check_bounds(s, got)


def test_consumer_reads_only_what_the_producer_wrote():
    """A workspace full of bf16 NaNs gives the bits of a zero-filled one."""
    c, s = WS_CASE, _setup(WS_CASE)
    ws = _workspace(c, s["q"], s["k"])
    ws.zero_()
    zero, _ = _run(c, s, 7, ws)
    ws.view(torch.int16).fill_(0x7FC0)
    nan, names = _run(c, s, 7, ws)
    _assert_ran(names, EMIT)
    for n, a, b in zip(("dq", "dk", "dv"), nan, zero):
        assert torch.isfinite(a.float()).all() and R.bits_equal(a, b), n


def test_workspace_reused_across_inputs():
    """Inputs A then inputs B on one workspace: B's result is that of a fresh workspace."""
    ca, cb = WS_CASE, _case("ds-256-causal-b", 256, 256, True, H=2)
    sa, sb = _setup(ca), _setup(cb)
    ws = _workspace(ca, sa["q"], sa["k"])
    _run(ca, sa, 7, ws)
    reused, _ = _run(cb, sb, 7, ws)
    fresh, _ = _run(cb, sb, 7, _workspace(cb, sb["q"], sb["k"]).zero_())
    for n, a, b in zip(("dq", "dk", "dv"), reused, fresh):
        assert R.bits_equal(a, b), n
    _check_bounds(sb, reused)


# ------------------------------------------------------------------------------------ fallbacks
def _ws_bytes(c):
    return _lib.require().kca_attn_bwd_ws_bytes(c["B"], c["Sq"], c["Sk"], c["H"], c["Hkv"], c["D"], int(c["causal"]))


def _some_ws(c):
    return torch.empty(c["B"] * c["H"] * c["Sq"] * c["Sk"] * 2, device=DEV, dtype=torch.uint8)


@pytest.mark.parametrize("how", ["none", "short", "variant3"])
def test_fallback_without_a_usable_workspace(how):
    c, s = WS_CASE, _setup(WS_CASE)
    assert _ws_bytes(c) == c["B"] * c["H"] * c["Sq"] * c["Sk"] * 2
    ws = {"none": None, "short": _some_ws(c)[:-1], "variant3": _some_ws(c)}[how]
    got, names = _run(c, s, 3 if how == "variant3" else 7, ws)
    _assert_ran(names, TWO_KERNEL)
    ref, _ = _run(c, s, 3, None)
    for n, a, b in zip(("dq", "dk", "dv"), got, ref):
        assert R.bits_equal(a, b), n


@pytest.mark.parametrize("c,kernels", [
    (_case("ds-gqa", 128, 384, True, H=4, Hkv=2), ("attn_bwd_dkdv_tiled_kernel", "attn_bwd_dq_tiled_kernel")),
    (_case("ds-d128", 256, 256, True, H=2, d=128), ("attn_bwd_dkdv_tiled_kernel", "attn_bwd_dq_tiled_kernel")),
], ids=["gqa", "d128"])
def test_fallback_outside_the_shape(c, kernels):
    s = _setup(c)
    assert _ws_bytes(c) == 0
    old = A.set_variant(7)
    try:
        assert A.bwd_workspace(s["q"], s["k"], True) is None
    finally:
        A.set_variant(old)
    got, names = _run(c, s, 7, _some_ws(c))
    _assert_ran(names, kernels)
    ref, _ = _run(c, s, 3, None)
    for n, a, b in zip(("dq", "dk", "dv"), got, ref):
        assert R.bits_equal(a, b), n


# ------------------------------------------------------------------------------------ through the ops
def _profiled(fn, variant):
    old = A.set_variant(variant)
    try:
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
    finally:
        A.set_variant(old)
    return out, sorted(set(e.name for e in prof.events() if "attn_bwd" in e.name and "preprocess" not in e.name))


def test_qkv_rope_attention():
    torch.manual_seed(5)
    B, S, H, rot = 1, 256, 2, 64
    qkv = torch.randn(B, S, 3 * H * D, device=DEV, dtype=BF16)
    g = torch.randn(B, S, H * D, device=DEV, dtype=BF16)

    def run():
        x = qkv.detach().clone().requires_grad_()
        ops.qkv_rope_attention(x * 1.0, H, D, rot, True).backward(g)
        return x.grad

    new, names = _profiled(run, 7)
    _assert_ran(names, EMIT)
    again, _ = _profiled(run, 7)
    ref, names3 = _profiled(run, 3)
    _assert_ran(names3, TWO_KERNEL)
    assert torch.equal(new, again), "two runs differ"
    if DQ_BIT_EQUAL:
        assert torch.equal(new, ref)
    else:
        assert torch.equal(new.view(B, S, 3, H, D)[:, :, 1:], ref.view(B, S, 3, H, D)[:, :, 1:])


def test_fused_parallel_block_backward():
    """One GPT-J block (2 heads of 256) through ops.fused_block: every gradient under variant 7 equals
    variant 3's."""
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import LMConfig, PRESETS_HF

    cfg = dict(PRESETS_HF["gpt-j-6b"])
    cfg.update(n_embd=512, n_layer=1, n_head=2, rotary_dim=64, vocab_size=512)
    model = build_model(LMConfig.from_hf(cfg), device=torch.device(DEV), dtype=BF16, seed=0)
    model.enable_tn_grads(True)
    assert model.h[0].fused is not None
    ids = torch.randint(0, 512, (1, 256), device=DEV, generator=torch.Generator(DEV).manual_seed(3))

    def run():
        model.zero_grad(set_to_none=True)
        model(ids, labels=ids).backward()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    new, names = _profiled(run, 7)
    _assert_ran(names, EMIT)
    ref, names3 = _profiled(run, 3)
    _assert_ran(names3, TWO_KERNEL)
    assert new.keys() == ref.keys() and any("qkv" in n for n in new)
    if DQ_BIT_EQUAL:
        for n in new:
            assert torch.equal(new[n], ref[n]), n
