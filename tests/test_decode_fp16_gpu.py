"""The fp16 decode kernels (the ``*_f16`` entries of csrc/kernels/gemv.hip, decode.hip, elementwise.hip and
the sampler's fp16 logits mode) against fp64 references of the same operations, and ``skinny_linear``'s
input guards.

One bound for every comparison (``_within``): the fp16 inputs are upcast to fp64 and the operation is
computed there (``ref``); the same operation in fp32 torch on the device is ``y32``; the kernel's fp16
output ``y`` must satisfy, per element,

    |y - ref| <= 2^-10 * max(|ref|, 2^-14) + 4 * max|y32 - ref|

-- two fp16 units in the last place of the reference (one for the output rounding, one for a reference on
a rounding boundary) plus four times the error of a plain fp32-accumulating implementation on the same
inputs (four: the summation orders differ). Both terms come from the reference at run time. bf16 outputs
(the bias guard) use the same form with bf16's two units, 2^-7, and its smallest normal, 2^-126.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd.ops import _lib
from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops import gemv
from kubernetes_cloud_amd.ops.rope import rope_tables

from .test_decode_gpu import _paginate, _params

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
H16 = torch.float16
_FMT = {torch.float16: (2.0 ** -10, 2.0 ** -14), torch.bfloat16: (2.0 ** -7, 2.0 ** -126)}


def _within(y, ref, y32, what, mask=None):
    """The module docstring's bound; ``mask`` restricts it (and the fp32 error term) to those elements."""
    two_ulp, tiny = _FMT[y.dtype]
    assert y.shape == ref.shape == y32.shape, (y.shape, ref.shape, y32.shape)
    yd, ref, y32 = y.double(), ref.double(), y32.double()
    if mask is not None:
        yd, ref, y32 = yd[mask], ref[mask], y32[mask]
    assert bool(torch.isfinite(ref.to(y.dtype)).all()), what  # the inputs keep the reference inside the format
    e32 = (y32 - ref).abs().max().item()
    tol = two_ulp * ref.abs().clamp_min(tiny) + 4 * e32
    err = (yd - ref).abs()
    ok = err <= tol  # (a NaN output compares False)
    print(f"{what}: max err {err.max().item():.3e}, fp32 err {e32:.3e}, worst err/bound "
          f"{(err / tol).max().item():.3f}")
    assert bool(ok.all()), (what, int((~ok).sum()), err[~ok].max().item(), tol[~ok].min().item(), e32)


def _spy(monkeypatch):
    """Names of the native entry points launched through ``_lib.call``."""
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", call)
    return names


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(g, *shape, scale=1.0, dtype=H16):
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(dtype)


def _act(z, act):
    return F.gelu(z, approximate="tanh") if act == 1 else F.gelu(z) if act == 2 else z


def _linear_refs(x, w, b, act):
    """(fp64 reference, fp32 torch result) of act(x W^T + b)."""
    out = []
    for dt in (torch.float64, torch.float32):
        z = x.to(dt) @ w.to(dt).t()
        if b is not None:
            z = z + b.to(dt)
        out.append(_act(z, act))
    return out


# ------------------------------------------------------------------ 1. skinny_linear, fp16, one row
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", [(1027, 1000), (1024, 2048), (1026, 4104), (512, 14336)])
def test_skinny_linear_f16_m1(N, K, bias, monkeypatch):
    """gemv1_kernel<2, false, 1, 1>: odd N against two rows per workgroup, a K tail inside the 2048-wide
    step, one slab past two steps, BLOOM's K; every activation; nothing written past N."""
    g = _gen(N + K + bias)
    x, w = _randn(g, 1, K), _randn(g, N, K, scale=K ** -0.5)
    b = _randn(g, N) if bias else None
    names = _spy(monkeypatch)
    for act in (0, 1, 2):
        ys = torch.full((1, N + 8), float("nan"), device=dev, dtype=H16)
        y = gemv.skinny_linear(x, w, b, act, out=ys[:, :N])
        assert y.data_ptr() == ys.data_ptr()
        ref, y32 = _linear_refs(x, w, b, act)
        _within(y, ref, y32, f"gemv f16 N={N} K={K} bias={bias} act={act}")
        assert bool(torch.isnan(ys[:, N:]).all())  # nothing written past the row
    assert names == ["kca_skinny_gemm_f16"] * 3


def test_skinny_linear_f16_overflow():
    """Two outputs of about +7e4 / -7e4 in fp32 leave fp16's range: they come back as +inf / -inf exactly as
    the reference rounds, and their finite neighbours stay within the bound."""
    N, K = 1026, 1000
    g = _gen(5)
    x, w = _randn(g, 1, K), _randn(g, N, K, scale=K ** -0.5)
    xf = x.float()[0]
    w[100] = (7e4 * xf / (xf @ xf)).to(H16)
    w[901] = (-7e4 * xf / (xf @ xf)).to(H16)
    y = gemv.skinny_linear(x, w)
    ref, y32 = _linear_refs(x, w, None, 0)
    r16 = ref.to(H16)
    assert 6.9e4 < ref[0, 100].item() < 7.1e4 and -7.1e4 < ref[0, 901].item() < -6.9e4
    inf = torch.isinf(r16)
    assert inf.nonzero()[:, 1].tolist() == [100, 901]
    assert torch.equal(y[inf], r16[inf]) and y[0, 100].item() == math.inf and y[0, 901].item() == -math.inf
    _within(y, ref, y32, "gemv f16 overflow neighbours", mask=~inf)


def test_skinny_linear_f16_subnormal_weights():
    """A block of weights at 2^-20 (subnormal in fp16) against x = 2048: their 512 products add 1.0 to each of
    the first 16 outputs. The GEMV's v_dot2_f32_f16 must keep subnormal fp16 operands (it does on gfx950: the
    outputs match the plain reference, and are 1.0 away from the one with subnormal inputs flushed)."""
    N, K = 1024, 2048
    g = _gen(9)
    x, w = _randn(g, 1, K), _randn(g, N, K, scale=K ** -0.5)
    x[0, :512] = 2048.0
    w[:, :512] = 0
    w[:16, :512] = 2.0 ** -20
    assert float(w[0, 0]) == 2.0 ** -20
    y = gemv.skinny_linear(x, w)
    ref, y32 = _linear_refs(x, w, None, 0)
    flush = lambda t: torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)  # noqa: E731
    ref_ftz = _linear_refs(flush(x), flush(w), None, 0)[0]
    assert bool(((ref - ref_ftz)[0, :16] - 1.0).abs().max() < 1e-2)  # what flushing would lose
    print("subnormal block: |y - ref| %.3e, |y - flushed ref| %.3e" %
          ((y.double() - ref)[0, :16].abs().max().item(), (y.double() - ref_ftz)[0, :16].abs().max().item()))
    _within(y, ref, y32, "gemv f16 subnormal weights")


# ------------------------------------------------------------------ C. skinny_linear's input guards
def test_skinny_linear_f16_strided_x(monkeypatch):
    """x = big[:, ::2] has a column stride of 2; the fp16 GEMV reads x as contiguous, so the call must take the
    F.linear path."""
    N, K = 1024, 2048
    g = _gen(21)
    big, w = _randn(g, 1, 2 * K), _randn(g, N, K, scale=K ** -0.5)
    x = big[:, ::2]
    assert x.shape == (1, K) and x.stride(1) == 2
    names = _spy(monkeypatch)
    y = gemv.skinny_linear(x, w)
    ref, y32 = _linear_refs(x, w, None, 0)
    _within(y, ref, y32, "strided x f16")
    assert "kca_skinny_gemm_f16" not in names


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_skinny_linear_strided_bias(dtype, monkeypatch):
    """bias = big[::2]: both kernels are handed bias.data_ptr() alone, so a strided bias must take the F.linear
    path."""
    N, K = 1024, 2048
    g = _gen(22)
    x, w = _randn(g, 1, K, dtype=dtype), _randn(g, N, K, scale=K ** -0.5, dtype=dtype)
    b = _randn(g, 2 * N, dtype=dtype)[::2]
    assert b.shape == (N,) and not b.is_contiguous()
    names = _spy(monkeypatch)
    y = gemv.skinny_linear(x, w, b)
    ref, y32 = _linear_refs(x, w, b, 0)
    _within(y, ref, y32, f"strided bias {dtype}")
    assert not [n for n in names if n.startswith("kca_skinny_gemm")]
    yc = gemv.skinny_linear(x, w, b.contiguous())  # and the contiguous bias still runs the native kernel
    assert [n for n in names if n.startswith("kca_skinny_gemm")]
    _within(yc, ref, y32, f"contiguous bias {dtype}")


# ------------------------------------------------------------------ 2. ln_rows / embed_ln_rows, fp16
def _ln_refs(h, gamma, beta, eps):
    return [F.layer_norm(h.to(dt), (h.shape[-1],), gamma.to(dt), None if beta is None else beta.to(dt), eps)
            for dt in (torch.float64, torch.float32)]


@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("K", [1000, 4096, 14336])
@pytest.mark.parametrize("M", [1, 3])
def test_ln_rows_f16(M, K, nres, monkeypatch):
    """h = x + residuals is the fp32 sum rounded to fp16, bit for bit; xn = LN(h) within the bound. At M = 3
    the last row holds entries near +-3e4 (residual sum under 6e4): a kernel that sums or squares in fp16
    overflows on it."""
    g = _gen(M * 100 + K + nres)
    x = torch.randn(M, K, generator=g, device=dev)
    res = [torch.randn(M, K, generator=g, device=dev) for _ in range(nres)]
    if M == 3:
        sgn = torch.sign(torch.randn(K, generator=g, device=dev))
        x[2] = sgn * 3e4 * (0.9 + 0.1 * torch.rand(K, generator=g, device=dev))
        for r in res:
            r[2] = sgn * 1e4 * torch.rand(K, generator=g, device=dev)
    x, res = x.to(H16), [r.to(H16) for r in res]
    gamma = (1 + 0.1 * torch.randn(K, generator=g, device=dev)).to(H16)
    h32 = x.float()
    for r in res:
        h32 = h32 + r.float()
    assert float(h32.abs().max()) < 6e4
    h_ref = h32.to(H16)
    names = _spy(monkeypatch)
    for beta in (_randn(g, K, scale=0.1), None):
        xn, h = gemv.ln_rows(x, gamma, beta, 1e-5, res)
        assert torch.equal(h, h_ref)
        ref, y32 = _ln_refs(h_ref, gamma, beta, 1e-5)
        _within(xn, ref, y32, f"ln_rows f16 M={M} K={K} nres={nres} beta={beta is not None}")
    assert names == ["kca_ln_rows_f16"] * 2


@pytest.mark.parametrize("K", [1000, 4096, 14336])
@pytest.mark.parametrize("M", [1, 3])
def test_embed_ln_rows_f16(M, K, monkeypatch):
    """Row m is wte[prev[chain[m]]] where chain[m] >= 0, else wte[tokens[m]]; ids 0 and V - 1 included."""
    V = 50
    g = _gen(M + K)
    wte = _randn(g, V, K)
    gamma = (1 + 0.1 * torch.randn(K, generator=g, device=dev)).to(H16)
    if M == 3:
        tokens, chain, prev = [0, 17, V - 1], [-1, 1, -1], [3, V - 2]
    else:
        tokens, chain, prev = [V - 1], [0], [0]
    tokens = torch.tensor(tokens, device=dev, dtype=torch.int64)
    chain = torch.tensor(chain, device=dev, dtype=torch.int32)
    prev = torch.tensor(prev, device=dev, dtype=torch.int64)
    ids_chain = torch.where(chain >= 0, prev[chain.clamp(min=0).long()], tokens)
    assert not torch.equal(ids_chain, tokens)
    names = _spy(monkeypatch)
    n = 0
    for ids, ch, pv in ((tokens, None, None), (ids_chain, chain, prev)):
        for beta in (_randn(g, K, scale=0.1), None):
            xn, h = gemv.embed_ln_rows(wte, tokens, gamma, beta, 1e-5, ch, pv)
            assert torch.equal(h, wte[ids])
            ref, y32 = _ln_refs(wte[ids], gamma, beta, 1e-5)
            _within(xn, ref, y32, f"embed_ln_rows f16 M={M} K={K} chain={ch is not None} beta={beta is not None}")
            n += 1
    assert names == ["kca_embed_ln_rows_f16"] * n


# ------------------------------------------------------------------ 3. _linear_act's GELU pass
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("rows", [3, 20])
def test_linear_act_gelu_f16(rows, act, monkeypatch):
    """kca_gelu_fwd_f16 on pre-activations spanning +-12 (an identity weight hands x through F.linear
    unchanged), with +-0, subnormal inputs and inputs whose GELU is subnormal in fp16 (about -5.5 .. -4.2);
    then the same values, signed zeros included, through the entry point directly."""
    N = 4096
    x = torch.linspace(-12, 12, rows * N, device=dev).to(H16).view(rows, N)
    x[0, :10] = torch.tensor([0.0, -0.0, 6e-8, -6e-8, 3e-5, -3e-5, -4.2, -4.75, -5.25, -5.5], device=dev).to(H16)
    eye = torch.eye(N, device=dev, dtype=H16)
    u = F.linear(x, eye)
    assert torch.equal(u, x)  # (-0 == +0)
    names = _spy(monkeypatch)
    y = gemv._linear_act(x, eye, None, act)
    assert names == ["kca_gelu_fwd_f16"]
    ref, y32 = _act(u.double(), act), _act(u.float(), act)
    sub = (ref.abs() < 2.0 ** -14) & (ref != 0)
    assert int(sub.sum()) > 100  # the subnormal band is covered
    _within(y, ref, y32, f"linear_act gelu f16 rows={rows} act={act}")
    y2 = x.clone()
    _lib.call("kca_gelu_fwd_f16", y2.data_ptr(), y2.data_ptr(), y2.numel(), int(act == 1), _lib.stream())
    _within(y2, _act(x.double(), act), _act(x.float(), act), f"gelu_fwd_f16 direct rows={rows} act={act}")
    assert float(y2[0, 0]) == 0.0 and float(y2[0, 1]) == 0.0


# ------------------------------------------------------------------ 4. gemv_dual_ln, fp16
@pytest.mark.parametrize("N,K1,K2,two_ln", [(1024, 1024, 4096, False), (1536, 1536, 6144, True),
                                             (3584, 448, 0, False), (3584, 1792, 0, True)])
def test_gemv_dual_ln_f16(N, K1, K2, two_ln):
    """The four shape families of test_gemv_dual_ln_matches_reference at a quarter of their sizes. h_out
    against the unrounded fp64 / fp32 sums; xn (and xn2) = LayerNorm of the h_out the kernel stored, so a
    reference h' that rounds the other way on an fp16 boundary is not charged to the LayerNorm. Three
    launches, every counter re-armed."""
    g = _gen(N + K1)
    x1, w1 = _randn(g, 1, K1), _randn(g, N, K1, scale=K1 ** -0.5)
    x2, w2 = (_randn(g, 1, K2), _randn(g, N, K2, scale=K2 ** -0.5)) if K2 else (None, None)
    b, h = _randn(g, N), _randn(g, 1, N)
    gamma, beta, g2, b2 = (_randn(g, N) for _ in range(4))
    ypart = torch.empty(N, device=dev, dtype=torch.float32)
    cnt = torch.zeros(32 * 65, device=dev, dtype=torch.int32)
    hs = []
    for dt in (torch.float64, torch.float32):
        y = x1.to(dt) @ w1.to(dt).t()
        if K2:
            y = y + x2.to(dt) @ w2.to(dt).t()
        hs.append(h.to(dt) + (y + b.to(dt)))
    hn32, _ = dops.gemv_dual_ln_reference(x1, w1, x2, w2, b, h, gamma, beta, 1e-5)
    assert hn32.dtype == H16
    for rep in range(3):
        h_out, xn, xn2 = (torch.full((1, N), float("nan"), device=dev, dtype=H16) for _ in range(3))
        dops.gemv_dual_ln(x1, w1, x2, w2, b, h, gamma, beta, 1e-5, ypart, cnt, h_out, xn,
                          *((g2, b2, xn2) if two_ln else (None, None, None)))
        torch.cuda.synchronize()
        _within(h_out, hs[0], hs[1], f"gemv_dual_ln f16 h' N={N} rep={rep}")
        _within(h_out, hs[0], hn32.float(), f"gemv_dual_ln f16 h' vs gemv_dual_ln_reference N={N} rep={rep}")
        ref, y32 = _ln_refs(h_out, gamma, beta, 1e-5)
        _within(xn, ref, y32, f"gemv_dual_ln f16 xn N={N} rep={rep}")
        if two_ln:
            ref, y32 = _ln_refs(h_out, g2, b2, 1e-5)
            _within(xn2, ref, y32, f"gemv_dual_ln f16 xn2 N={N} rep={rep}")
    assert int(cnt.abs().sum()) == 0  # every counter re-armed


# ------------------------------------------------------------------ 5./6. fused prep + attention, fp16
def _attention64(q, kc, vc, slots, lens, H, scale, alibi, tbl):
    """decode_attention_reference's math in fp64."""
    B, Hkv, D = q.shape[0], kc.shape[1], kc.shape[3]
    out = torch.empty(B, H * D, device=q.device, dtype=torch.float64)
    for b in range(B):
        n, s = int(lens[b]), int(slots[b])
        qb = q[b, :H * D].double().view(H, D)
        kb = dops.gather_kv(kc, s, n, tbl).double().repeat_interleave(H // Hkv, 0)
        vb = dops.gather_kv(vc, s, n, tbl).double().repeat_interleave(H // Hkv, 0)
        sc = torch.einsum("hd,hnd->hn", qb, kb) * scale
        if alibi is not None:
            sc = sc + alibi.double()[:, None] * (torch.arange(n, device=q.device) - (n - 1)).double()[None]
        out[b] = torch.einsum("hn,hnd->hd", sc.softmax(-1), vb).reshape(-1)
    return out


def _prep_attention_refs(qkv, kc, vc, H, Hkv, D, rot, inter, cos, sin, pos, slots, kl, alibi, tbl):
    """The module's reference path (decode_prep's torch branch, decode_attention_reference) on fp32 upcasts,
    with the roundings the fp16 operation stores: the appended K / V rows and the rotated Q (the two-kernel
    path rotates Q in place in the fp16 buffer) are rounded to fp16 before the attention.
    Returns (K cache, V cache in fp16, fp64 output, fp32 output)."""
    q32, k32, v32 = qkv.float(), kc.float(), vc.float()
    dops.decode_prep(q32, H, Hkv, D, rot, inter, cos, sin, pos, slots, k32, v32, tbl)
    q16, k16, v16 = q32.to(H16), k32.to(H16), v32.to(H16)
    scale = 1 / math.sqrt(D)
    y32 = dops.decode_attention_reference(q16.float(), k16.float(), v16.float(), slots, kl, H, scale, alibi,
                                          torch.empty(qkv.shape[0], H * D, device=dev), tbl)
    return k16, v16, _attention64(q16, k16, v16, slots, kl, H, scale, alibi, tbl), y32


def _attn_case(B, Hkv, G, D, L, PS, seed):
    g = _gen(seed)
    H = Hkv * G
    kc, vc = _randn(g, B + 1, Hkv, L, D), _randn(g, B + 1, Hkv, L, D)
    tbl = None
    if PS:
        kc, tbl = _paginate(kc, PS, 3)
        vc, _ = _paginate(vc, PS, 3)
    return H, kc, vc, tbl, _randn(g, B, (H + 2 * Hkv) * D)


@pytest.mark.parametrize("D,rot,inter,G,PS,alibi", [(256, 64, True, 1, 64, False), (128, 32, False, 4, 0, False),
                                                    (80, 20, False, 1, 0, False), (64, 0, False, 2, 32, False),
                                                    (128, 0, False, 1, 0, True)])
def test_decode_prep_attention_f16(D, rot, inter, G, PS, alibi, monkeypatch):
    """kca_decode_prep_attn_f16: the appended K / V rows equal the reference's rows rounded to fp16, the
    attention output is within the bound, the QKV buffer is untouched. Positions 0, L - 1 and both sides of
    a 64-token chunk edge."""
    B, Hkv, L = 5, 4, 512
    H, kc, vc, tbl, qkv = _attn_case(B, Hkv, G, D, L, PS, D + rot + G)
    slots = torch.tensor([3, 0, 5, 1, 2], device=dev, dtype=torch.int32)
    pos = torch.tensor([0, L - 1, 200, 63, 64], device=dev, dtype=torch.int32)
    kl = pos + 1
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    al = None
    if alibi:
        from kubernetes_cloud_amd.models.causal_lm import alibi_slopes
        al = alibi_slopes(H).to(dev)
    kk, vk, qk = kc.clone(), vc.clone(), qkv.clone()
    names = _spy(monkeypatch)
    o = dops.decode_prep_attention(qk, H, Hkv, D, rot, inter, cos, sin, pos, slots, kk, vk, kl, L, alibi=al,
                                   block_table=tbl)
    torch.cuda.synchronize()
    assert names == ["kca_decode_prep_attn_f16"]
    k16, v16, ref, y32 = _prep_attention_refs(qkv, kc, vc, H, Hkv, D, rot, inter, cos, sin, pos, slots, kl, al, tbl)
    assert torch.equal(vk, v16)
    assert torch.equal(kk, k16)
    assert torch.equal(qk, qkv)  # the fused kernel leaves the QKV buffer untouched
    _within(o, ref, y32, f"decode_prep_attention f16 D={D} rot={rot} G={G} page={PS} alibi={alibi}")


@pytest.mark.parametrize("D,rot,H,alibi", [(256, 64, 4, False), (128, 0, 8, True)])
def test_decode_prep_attention_gemv_f16(D, rot, H, alibi):
    """kca_decode_prep_attn_gemv_f16 (batch 1): the attention workgroups against the fused-attention
    reference, the GEMV workgroups against the GEMV reference (odd N, K tail, bias + GELU)."""
    L, N, K = 512, 1027, 1000
    _, kc, vc, tbl, qkv = _attn_case(1, H, 1, D, L, 0, D + H)
    g = _gen(D)
    gx, gw, gb = _randn(g, 1, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    slots = torch.tensor([1], device=dev, dtype=torch.int32)
    pos = torch.tensor([300], device=dev, dtype=torch.int32)
    kl = pos + 1
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    al = None
    if alibi:
        from kubernetes_cloud_amd.models.causal_lm import alibi_slopes
        al = alibi_slopes(H).to(dev)
    ws = torch.zeros(max(dops.decode_ws_floats(1, H, H, D, L), 1), device=dev, dtype=torch.float32)
    kk, vk, qk = kc.clone(), vc.clone(), qkv.clone()
    out = torch.full((1, H * D), float("nan"), device=dev, dtype=H16)
    gy = torch.full((1, N), float("nan"), device=dev, dtype=H16)
    assert dops.decode_prep_attention_gemv(qk, H, H, D, rot, True, cos, sin, pos, slots, kk, vk, kl, L, D ** -0.5,
                                           al, out, ws, tbl, 0, gx, gw, gb, gy, 1)
    torch.cuda.synchronize()
    k16, v16, ref, y32 = _prep_attention_refs(qkv, kc, vc, H, H, D, rot, True, cos, sin, pos, slots, kl, al, tbl)
    assert torch.equal(vk, v16)
    assert torch.equal(kk, k16)
    assert torch.equal(qk, qkv)
    _within(out, ref, y32, f"decode_prep_attention_gemv f16 attention D={D} alibi={alibi}")
    gref, g32 = _linear_refs(gx, gw, gb, 1)
    _within(gy, gref, g32, f"decode_prep_attention_gemv f16 gemv D={D}")


# ------------------------------------------------------------------ 7. sampler, fp16 logits
def test_sample_f16_greedy_and_masks():
    """test_sample_greedy_and_masks' assertions on fp16 logits at V = 1000, with a row holding -inf entries, a
    row holding 65504 and banned ids (one of them a row's best token)."""
    torch.manual_seed(0)
    B, V = 8, 1000
    logits = (torch.randn(B, V, device=dev) * 4).to(H16)
    logits[2, 5:400:7] = float("-inf")
    logits[3, 123] = 65504.0
    bans = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    bans[1, 0] = logits[1].float().argmax()
    bans[5, 1] = 17
    proc = lambda t: dops.processed_logits_reference(logits, torch.full((B,), t), None, None, None, bans)  # noqa: E731
    ids, lp = dops.sample_logits(logits, **_params(B, 0.0, 0, 1.0), ban_ids=bans)
    x = proc(0.0)
    ref = x.argmax(-1)
    assert torch.equal(ids, ref)
    assert int(ids[1]) != int(bans[1, 0]) and int(ids[3]) == 123
    assert torch.allclose(lp, torch.log_softmax(x, -1).gather(1, ref[:, None])[:, 0], atol=1e-3)
    for (t, k, p) in ((1.0, 50, 1.0), (0.7, 0, 0.9), (1.3, 40, 0.8), (1.0, 1, 1.0), (1.0, 0, 0.5)):
        kept = torch.empty(B, dtype=torch.int32, device=dev)
        ids, _ = dops.sample_logits(logits, **_params(B, t, k, p), seeds=torch.arange(B, device=dev),
                                    out_kept=kept, ban_ids=bans)
        x = proc(t)
        for b in range(B):
            keep = dops.keep_mask_reference(x[b], k, p)
            # (ties with the threshold value are all kept by the kernel, see test_sample_greedy_and_masks)
            expect = int((x[b] >= x[b][keep].min()).sum())
            assert int(keep.sum()) <= int(kept[b]) <= expect + max(1, expect // 100), (t, k, p, b)
            assert bool(keep[ids[b]]), (t, k, p, b)
