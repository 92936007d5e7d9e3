"""The 8-wave (two waves per SIMD) D = 256 dK/dV kernel, bit 1 of kca_attn_set_variant
(attn_bwd_dkdv_w8_kernel, csrc/kernels/attention_tiled.hip), against the 4-wave kernel and an fp32
reference. A pair of waves splits dV / dK of 32 keys and the dK wave runs one Q tile behind through
three Q/dO buffers, so the shapes cover two and three key blocks (buffer rotation), the bottom-right
causal offset, a long loop, the fused-QKV strides and the GQA fallback. The kernel keeps the 4-wave
kernel's MFMA shapes, fp32 P and accumulation order: dK and dV must be bit-identical to it."""
import pytest
import torch

from kubernetes_cloud_amd import ops
from kubernetes_cloud_amd.ops.attention import set_variant

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _grads(var, q, k, v, g, causal):
    """dQ, dK, dV of ops.flash_attention under variant bits `var` (fresh leaves, same values)."""
    old = set_variant(var)
    try:
        ql, kl, vl = (t.detach().clone().requires_grad_() for t in (q, k, v))
        ops.flash_attention(ql, kl, vl, causal=causal).backward(g)
        torch.cuda.synchronize()
        return ql.grad, kl.grad, vl.grad
    finally:
        set_variant(old)


def _case(B, Sq, Sk, H, Hkv, causal, bit_identical=True):
    torch.manual_seed(7)
    q = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, Sk, Hkv, D, device=DEV, dtype=torch.bfloat16)
    v = torch.randn(B, Sk, Hkv, D, device=DEV, dtype=torch.bfloat16)
    g = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16)
    new = _grads(3, q, k, v, g, causal)
    again = _grads(3, q, k, v, g, causal)
    old = _grads(1, q, k, v, g, causal)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    orf, _ = ops.attention_reference(qr, kr, vr, causal)
    orf.backward(g.float())
    for name, got, ref in zip(("dq", "dk", "dv"), new, (qr.grad, kr.grad, vr.grad)):
        print(name, "vs fp32", _rel(got, ref))
        assert _rel(got, ref) < 3e-2, (name, _rel(got, ref))
    assert torch.equal(new[0], old[0]), "dq: its kernel is unchanged"
    for name, a, b, c in zip(("dk", "dv"), new[1:], old[1:], again[1:]):
        print(name, "vs 4-wave", _rel(a, b), "max abs", (a.float() - b.float()).abs().max().item())
        if bit_identical:
            assert torch.equal(a, b), (name, "differs from the 4-wave kernel", _rel(a, b))
        assert torch.equal(a, c), (name, "differs between two runs")


@pytest.mark.parametrize("causal", [True, False])
def test_two_key_blocks(causal):
    _case(2, 256, 256, 2, 2, causal)


@pytest.mark.parametrize("causal", [True, False])
def test_three_key_blocks_buffer_rotation(causal):
    _case(1, 384, 384, 2, 2, causal)   # 12 / 8 / 4 Q tiles under the mask


def test_causal_bottom_right_offset():
    _case(1, 128, 384, 2, 2, True)     # offset 256: only the last key block is masked


def test_long_loop():
    _case(1, 1024, 1024, 1, 1, True)   # 32 Q tiles on the first key block


def test_gqa_keeps_the_4wave_kernel():
    """H != Hkv is outside the 8-wave kernel: with bit 1 set the dispatch must still take the 4-wave
    kernel (which sweeps the query heads of a KV head) and match the reference."""
    _case(1, 128, 384, 4, 2, True)


def test_fused_qkv_strides_and_dk_unrotation():
    """ops.qkv_rope_attention: Q/K/V read from, and dQ/dK/dV written into, the fused [B, S, 3, H, D]
    buffers (token stride 3 H D), dQ/dK un-rotated in place afterwards."""
    torch.manual_seed(5)
    B, S, H, rot = 1, 256, 2, 64
    qkv = torch.randn(B, S, 3 * H * D, device=DEV, dtype=torch.bfloat16)
    g = torch.randn(B, S, H * D, device=DEV, dtype=torch.bfloat16)

    def run(var):
        old = set_variant(var)
        try:
            x = qkv.detach().clone().requires_grad_()
            ops.qkv_rope_attention(x * 1.0, H, D, rot, True).backward(g)
            torch.cuda.synchronize()
            return x.grad.view(B, S, 3, H, D)
        finally:
            set_variant(old)

    new, again, old = run(3), run(3), run(1)
    xr = qkv.float().cpu().requires_grad_()
    ops.qkv_rope_attention(xr, H, D, rot, True).backward(g.float().cpu())
    ref = xr.grad.view(B, S, 3, H, D)
    for i, name in enumerate(("dq", "dk", "dv")):
        r = _rel(new[:, :, i].cpu(), ref[:, :, i])
        print(name, "vs fp32", r)
        assert r < 3e-2, (name, r)
    assert torch.equal(new[:, :, 0], old[:, :, 0]), "dq: its kernel is unchanged"
    for i, name in ((1, "dk"), (2, "dv")):
        assert torch.equal(new[:, :, i], old[:, :, i]), (name, "differs from the 4-wave kernel")
        assert torch.equal(new[:, :, i], again[:, :, i]), (name, "differs between two runs")
