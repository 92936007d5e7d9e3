"""MXFP4 weight-only decode on CPU (ops/mx4.py reference paths, the engine option): the quantizer
against an independent numpy / fp64 derivation of the OCP rule on planted blocks, the byte-exact round
trips, the linear's reference against fp64, and ``LLMEngine(weight_dtype="mxfp4")`` runs whose tokens
match the model's own forward."""
import math

import numpy as np
import pytest
import torch

from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.models.causal_lm import build_model
from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
from kubernetes_cloud_amd.ops import mx4

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}


def _np_quantize(w: torch.Tensor):
    """The format's rule written out per block and element in Python floats (fp64): returns (codes
    [N, K] with the sign in bit 3, scale bytes [N, K/32])."""
    a = w.double().numpy()
    N, K = a.shape
    codes = np.zeros((N, K), dtype=np.uint8)
    scale = np.zeros((N, K // 32), dtype=np.uint8)
    for n in range(N):
        for b in range(K // 32):
            blk = a[n, 32 * b:32 * b + 32]
            fin = np.where(np.isfinite(blk), blk, 0.0)
            amax = float(np.abs(fin).max())
            if amax == 0.0:
                e = 0
            else:
                m, ex = math.frexp(amax)  # amax = m 2^ex, 0.5 <= m < 1
                e = min(127, max(-127, (ex - 1) - 2))
            scale[n, b] = e + 127
            for i in range(32):
                v = min(abs(float(fin[i])) / 2.0 ** e, 6.0)  # exact: a 24-bit significand over a power of two
                d = [abs(v - g) for g in GRID]
                best = min(d)
                c = [j for j in range(8) if d[j] == best]
                c = c[0] if len(c) == 1 else [j for j in c if j % 2 == 0][0]  # a tie: the even code
                neg = bool(np.signbit(blk[i])) and bool(np.isfinite(blk[i]))
                codes[n, 32 * b + i] = c | (8 if neg else 0)
    return codes, scale


def _planted(dtype, seed=0):
    """[14, 96]: random rows at several magnitudes plus planted blocks (row, block): (2, 0) all zeros,
    (3, 1) amax exactly 2^-2, (4, 0) amax just below one, (5, 2) the seven ties under a scale of one,
    (6, 1) amax 7 * 2^-3 (saturates to +-6), (7, 0) -0.0 elements, (8, 2) non-finite elements, (9, 0)
    the largest finite values of the type, (10, 1) tiny values."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(14, 96, generator=g) * torch.logspace(-6, 3, 14)[:, None]
    w[2, :32] = 0.0
    w[3, 32:64] = torch.randn(32, generator=g).clamp(-1, 1) * 0.2
    w[3, 40] = 0.25
    w[4, :32] = torch.rand(32, generator=g) * 0.9
    w[4, 5] = -0.9921875  # 127/128: exact in bf16 and fp16
    ties = list(TIES) + [-t for t in TIES]
    w[5, 64:96] = 0.0
    w[5, 64:64 + len(ties)] = torch.tensor(ties)
    w[5, 95] = 6.0  # amax in [4, 8): the block's scale is 2^0
    w[6, 32:64] = torch.rand(32, generator=g) * 0.5
    w[6, 33], w[6, 34] = 0.875, -0.875
    w[7, 3], w[7, 8] = -0.0, -0.0
    w[8, 64], w[8, 65], w[8, 66] = float("nan"), float("inf"), float("-inf")
    big = torch.finfo(dtype).max
    w[9, :32] = torch.randn(32, generator=g) * big * 0.1
    w[9, 1], w[9, 2] = big, -big
    w[10, 32:64] = torch.randn(32, generator=g) * 1e-30
    return w.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_quantizer_against_numpy(dtype):
    w = _planted(dtype)
    q = mx4.quantize_weight(w)
    N, K = w.shape
    assert q.q.dtype == torch.uint8 and q.q.shape == (N, K // 2) and q.q.is_contiguous()
    assert q.scale.dtype == torch.uint8 and q.scale.shape == (N, K // 32) and q.scale.is_contiguous()
    assert q.shape == w.shape and q.nbytes() == N * K // 2 + N * K // 32
    codes, scale = _np_quantize(w)
    assert np.array_equal(q.scale.numpy(), scale)
    got = torch.stack((q.q & 0xF, q.q >> 4), dim=2).reshape(N, K).numpy()
    assert np.array_equal(got, codes)
    assert not (q.scale == 0xFF).any()
    # the planted blocks, spelled out
    assert int(q.scale[2, 0]) == 127 and not q.q[2, :16].any()
    assert int(q.scale[3, 1]) == 127 - 2 - 2 and got[3, 40] == 6  # 0.25 = 4 * 2^-4
    assert int(q.scale[4, 0]) == 127 - 1 - 2 and got[4, 5] == 0xF  # -0.992 / 2^-3 = -7.9 -> -6
    assert int(q.scale[5, 2]) == 127
    val = q.values(torch.float64)
    for i, (t, r) in enumerate(TIES.items()):
        assert float(val[5, 64 + i]) == r and float(val[5, 64 + len(TIES) + i]) == -r, t
    assert int(q.scale[6, 1]) == 127 - 1 - 2 and got[6, 33] == 0x7 and got[6, 34] == 0xF  # 7 * 2^-3 -> +-6 * 2^-3
    assert got[7, 3] == 0x8 and got[7, 8] == 0x8  # the sign of -0.0 is kept
    assert (got[8, 64:67] == 0).all()  # non-finite: +0
    assert got[9, 1] in (0x6, 0x7) and got[9, 2] in (0xE, 0xF)
    # dequantize is value * 2^(E - 127), formed in fp32
    s = torch.from_numpy(np.ldexp(1.0, scale.astype(np.int64) - 127))
    assert torch.equal(q.scales(torch.float64), s)
    full = val.view(N, -1, 32) * s[:, :, None]
    assert torch.equal(mx4.dequantize(q).double(), full.view(N, K).float().double())
    # half a step of the grid: relative 1/4 at worst (between 1 and 1.5 ... ), 0.25 absolute below 0.5,
    # one step (2 of 6) where the block saturates
    wd = torch.nan_to_num(w.double(), nan=0.0, posinf=0.0, neginf=0.0).view(N, -1, 32) / s[:, :, None]
    err = (val.view(N, -1, 32) - wd).abs()
    assert (err <= torch.maximum(wd.abs() / 4, torch.tensor(0.25, dtype=torch.float64))).all()


def test_packing_low_nibble_first():
    """One nonzero per row at a distinct k, odd and even: 1.0 in an otherwise zero block is 4 * 2^-2."""
    ks = [0, 1, 2, 33, 62, 63, 31, 32]
    w = torch.zeros(len(ks), 64)
    for n, k in enumerate(ks):
        w[n, k] = 1.0 if n % 2 == 0 else -1.0
    q = mx4.quantize_weight(w)
    want_q = torch.zeros(len(ks), 32, dtype=torch.uint8)
    want_s = torch.full((len(ks), 2), 127, dtype=torch.uint8)
    for n, k in enumerate(ks):
        want_q[n, k // 2] = (0x6 if n % 2 == 0 else 0xE) << (4 * (k & 1))
        want_s[n, k // 32] = 125
    assert torch.equal(q.q, want_q) and torch.equal(q.scale, want_s)
    assert torch.equal(mx4.dequantize(q), w)


def test_rejects_k_off_the_block():
    with pytest.raises(ValueError, match="K % 32"):
        mx4.quantize_weight(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        mx4.quantize_weight(torch.zeros(64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_round_trips(dtype):
    w = _planted(dtype, seed=1)
    if dtype == torch.float16:
        w = w[:10]  # (row 10's 1e-30 block is zero in fp16 already; keep the docstring's fp16 range)
    q = mx4.quantize_weight(w)
    q2 = mx4.quantize_weight(mx4.dequantize(q))
    assert torch.equal(q2.q & 0x77, q.q & 0x77) and torch.equal(q2.scale, q.scale)
    assert torch.equal(q2.q, q.q)  # signed zeros included
    snap = mx4.snap_to_grid(w)
    assert snap.dtype == dtype
    assert torch.equal(mx4.snap_to_grid(snap).view(torch.uint8), snap.view(torch.uint8))
    q3 = mx4.quantize_weight(snap)
    assert torch.equal(q3.q, q.q) and torch.equal(q3.scale, q.scale)
    # exact in bf16: the fp32 product survives the cast unchanged
    d32 = mx4.dequantize(q, torch.float32)
    assert torch.equal(mx4.dequantize(q, torch.bfloat16).float(), d32)
    if dtype != torch.float32:
        assert torch.equal(snap.float(), d32)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_against_fp64(dtype, act):
    g = torch.Generator().manual_seed(2)
    M, N, K = 5, 24, 96
    q = mx4.quantize_weight(torch.randn(N, K, generator=g) * 0.05)
    x = torch.randn(M, K, generator=g).to(dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(dtype)
    wd = mx4.dequantize(q).double()  # exact
    ref = torch.nn.functional.linear(x.double(), wd, b.double())
    if act:
        ref = torch.nn.functional.gelu(ref, approximate="tanh" if act == 1 else "none")
    got = mx4.mx4_linear_reference(x, q, b, act)
    assert got.dtype == dtype
    # one output rounding (half an ulp of the type) + fp32 accumulation noise on |x|.|w| (GELU' <= 1.13)
    eps = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    mag = torch.nn.functional.linear(x.double().abs(), wd.abs(), b.double().abs())
    tol = eps * ref.abs() + 1.13 * 2.0 ** -20 * mag + 2.0 ** -25
    assert ((got.double() - ref).abs() <= tol).all()
    got64 = mx4.mx4_linear_reference(x, q, b, act, fp64=True)
    assert ((got64.double() - ref).abs() <= eps * ref.abs() + 2.0 ** -40).all()
    # mx4_linear on CPU tensors is the reference path; `out` is filled in place
    out = torch.zeros(M, N, dtype=dtype)
    assert mx4.mx4_linear(x, q, b, act, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="K = 64"):
        mx4.mx4_linear(x[:, :64], q)


SMALL = {"gpt-j-6b": dict(n_embd=64, n_layer=2, n_head=4, rotary_dim=8, n_positions=64),
         "bloom-560m": dict(hidden_size=64, n_layer=2, n_head=4)}


def _tiny(preset, vocab=97, **over):
    cfg = dict(PRESETS_HF[preset])
    cfg.update(SMALL[preset])
    cfg.update(vocab_size=vocab, **over)
    m = build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)
    with torch.no_grad():  # grid weights: MXFP4 is lossless, prefill (full precision) and decode agree
        for blk in m.h:
            for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out):
                if mod.weight.shape[1] % 32 == 0:
                    mod.weight.copy_(mx4.snap_to_grid(mod.weight))
    return m


def _check_against_forward(m, prompt, out, margin):
    """Every generated token with a clear top-2 margin in the model's full forward is that forward's
    argmax; returns how many tokens were checked."""
    with torch.no_grad():
        lg = m(torch.tensor([prompt + out]))[0].float()
    n = 0
    for i, t in enumerate(out):
        row = lg[len(prompt) - 1 + i]
        top2 = row.topk(2).values
        if float(top2[0] - top2[1]) > margin:
            assert int(row.argmax()) == t, i
            n += 1
    return n


@pytest.mark.parametrize("preset", list(SMALL))
def test_engine_mxfp4_matches_forward(preset):
    m = _tiny(preset)
    prompts = [[5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8, 9], [11, 12, 13]]
    eng = LLMEngine(m, max_slots=4, max_len=48, weight_dtype="mxfp4")
    r = eng.runner
    assert r._w8 is None and r._mx4 is not None and len(r._mx4) == 4 * len(m.h)
    for blk in m.h:  # snapped weights quantize to themselves
        assert torch.equal(mx4.dequantize(r._mx4[id(blk.mlp.fc_out)]), blk.mlp.fc_out.weight)
    reqs = eng.generate(prompts, SamplingParams(max_new_tokens=8, do_sample=False))
    assert r.mx4_steps > 0 and r.w8_steps == 0 and r.batched_steps == 0 and r.fused_steps == 0
    checked = sum(_check_against_forward(m, p, q.output, margin=0.1) for p, q in zip(prompts, reqs))
    # fp32 model, lossless weights: the two paths differ by fp32 summation order only, far inside the
    # margin; the tighter margin of the FP8 twin of this test checks (nearly) every token
    tight = sum(_check_against_forward(m, p, q.output, margin=1e-4) for p, q in zip(prompts, reqs))
    print(f"{preset}: {checked} (margin 0.1) / {tight} (margin 1e-4) of 24 tokens checked")
    assert tight >= 12  # at least half of the 24 generated tokens


def test_engine_option_env_and_values(monkeypatch):
    m = _tiny("gpt-j-6b")
    monkeypatch.delenv("KCA_DECODE_WEIGHTS", raising=False)
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.runner._mx4 is None and eng.runner._w8 is None
    eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))
    assert eng.runner.mx4_steps == 0
    monkeypatch.setenv("KCA_DECODE_WEIGHTS", "mxfp4")
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.runner._mx4 is not None and eng.runner._w8 is None
    out = eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))[0].output
    assert eng.runner.mx4_steps > 0 and eng.runner.w8_steps == 0 and len(out) == 3
    # the keyword wins over the environment
    eng = LLMEngine(m, max_slots=2, max_len=32, weight_dtype="fp8")
    assert eng.runner._w8 is not None and eng.runner._mx4 is None
    monkeypatch.setenv("KCA_DECODE_WEIGHTS", "0")
    assert LLMEngine(m, max_slots=2, max_len=32).runner._mx4 is None
    for bad in ("fp4", "int3", "mxfp6"):
        with pytest.raises(ValueError, match=r"weight_dtype / KCA_DECODE_WEIGHTS.*'fp8', 'mxfp4'"):
            LLMEngine(m, max_slots=2, max_len=32, weight_dtype=bad)


def test_engine_mxfp4_composes_with_fp8_kv():
    m = _tiny("gpt-j-6b")
    eng = LLMEngine(m, max_slots=2, max_len=48, weight_dtype="mxfp4", kv_dtype="fp8")
    out = eng.generate([[1, 2, 3, 4]], SamplingParams(max_new_tokens=4, do_sample=False))[0].output
    assert len(out) == 4 and eng.runner.mx4_steps > 0 and eng.runner.kv8_steps > 0


def test_engine_mxfp4_refusals():
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=64, n_layer=2, n_head=4, vocab_size=96)
    tp = emulated_rank_model(LMConfig.from_hf(cfg), 2, 0, dtype=torch.float32)
    with pytest.raises(ValueError, match="mxfp4.*tensor-parallel.*serve this model with 16-bit weights$"):
        LLMEngine(tp, max_slots=2, max_len=32, weight_dtype="mxfp4")
    m = _tiny("gpt-j-6b")
    m.h[1].to("meta")  # a second device under the last layer: a layer-split placement
    with pytest.raises(ValueError, match="mxfp4.*layer-split.*serve this model with 16-bit weights$"):
        LLMEngine(m, max_slots=2, max_len=32, weight_dtype="mxfp4")
    odd = _tiny("gpt-j-6b", n_embd=48)  # K = 48 on qkv / out / fc_in
    with pytest.raises(ValueError, match="mxfp4.*K = 48.*serve this model with 16-bit weights$"):
        LLMEngine(odd, max_slots=2, max_len=32, weight_dtype="mxfp4")
    assert LLMEngine(odd, max_slots=2, max_len=32).runner._mx4 is None  # 16-bit weights do serve it
