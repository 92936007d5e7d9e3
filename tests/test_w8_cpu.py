"""FP8 weight-only decode on CPU (ops/w8.py reference paths, the engine option): quantizer properties
on random and planted rows, the lossless grid round trip, the linear's reference against fp64, and an
``LLMEngine(weight_dtype="fp8")`` run whose tokens match the model's own forward."""
import pytest
import torch

from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.models.causal_lm import build_model
from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
from kubernetes_cloud_amd.ops import w8


def _planted(K=96, seed=0):
    """Random rows plus: an all-zero row, a row whose absmax element is negative, a row with values
    below the e4m3 subnormal step (2^-9) after scaling, a row containing -0.0. Returns (w, row index
    of each plant)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(12, K, generator=g) * 0.05
    w[3] = 0.0
    w[5, 7] = -1.5  # |.| far above the rest of the row
    w[6] = torch.randn(K, generator=g) * 1e-7  # scale = 1/448 -> quotients ~4e-5, far below 2^-9 / 2
    w[6, 0] = 1.0
    w[8, 2] = -0.0
    w[8, 9] = -0.0
    return w, dict(zero=3, neg=5, tiny=6, negzero=8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_quantizer_properties(dtype):
    w, rows = _planted()
    w = w.to(dtype)
    q = w8.quantize_weight(w)
    assert q.q.dtype == torch.uint8 and q.q.shape == w.shape and q.q.is_contiguous()
    assert q.scale.dtype == torch.float32 and q.scale.shape == (w.shape[0],)
    assert not ((q.q == 0x7F) | (q.q == 0xFF)).any()
    wd = w.double()
    sc = q.scale.double()[:, None]
    # scale = absmax / 448 formed in fp32
    amax = w.float().abs().amax(dim=1)
    assert torch.equal(q.scale, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)))
    # half an e4m3 ulp: 3 mantissa bits -> 2^-4 relative; subnormal step 2^-9 -> 2^-10 absolute
    err = (q.values(torch.float64) * sc - wd).abs()
    bound = sc * 2.0 ** -4 * torch.maximum((wd / sc).abs(), torch.tensor(2.0 ** -6, dtype=torch.float64))
    assert (err <= bound).all(), float((err - bound).max())
    assert float(q.scale[rows["zero"]]) == 1.0 and not q.q[rows["zero"]].any()
    assert int(q.q[rows["neg"], 7]) == 0xFE  # -448: sign | exponent 1111 | mantissa 110
    assert int(q.q[rows["tiny"], 0]) == 0x7E and (q.q[rows["tiny"], 1:] & 0x7F).max() == 0  # flushed to +-0
    assert int(q.q[rows["negzero"], 2]) == 0x80 and int(q.q[rows["negzero"], 9]) == 0x80
    # dequantize() is the same product rounded to the asked type
    assert torch.equal(w8.dequantize(q, torch.float32), (q.values(torch.float32) * q.scale[:, None]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_grid_round_trip_is_lossless(dtype):
    w, rows = _planted(K=64, seed=1)
    w = w.to(dtype)
    snap = w8.snap_to_grid(w)
    assert snap.dtype == dtype
    q = w8.quantize_weight(snap)
    amax = w.float().abs().amax(dim=1)
    s = torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0))), torch.ones_like(amax))
    assert torch.equal(q.scale, s)
    back = w8.dequantize(q, dtype)
    assert torch.equal(back.view(torch.int16), snap.view(torch.int16))  # bitwise (signed zeros included)
    assert (q.values().abs().amax(dim=1)[amax > 0] == 448.0).all()
    assert not snap[rows["zero"]].any()


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_against_fp64(dtype, act):
    g = torch.Generator().manual_seed(2)
    M, N, K = 5, 24, 80
    q = w8.quantize_weight(torch.randn(N, K, generator=g) * 0.05)
    x = torch.randn(M, K, generator=g).to(dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(dtype)
    wd = q.values(torch.float64) * q.scale.double()[:, None]  # the dequantized weight, exact in fp64
    ref = torch.einsum("mk,nk->mn", x.double(), wd) + b.double()
    if act:
        ref = torch.nn.functional.gelu(ref, approximate="tanh" if act == 1 else "none")
    got = w8.w8_linear_reference(x, q, b, act)
    assert got.dtype == dtype
    # one output rounding (half an ulp of the type) + fp32 accumulation noise on |x|.|w| (GELU' <= 1.13)
    eps = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    mag = torch.einsum("mk,nk->mn", x.double().abs(), wd.abs()) + b.double().abs()
    tol = eps * ref.abs() + 1.13 * 2.0 ** -20 * mag + 2.0 ** -25
    assert ((got.double() - ref).abs() <= tol).all()
    # the fp64 form rounds the same contract
    got64 = w8.w8_linear_reference(x, q, b, act, fp64=True)
    assert ((got64.double() - ref).abs() <= eps * ref.abs() + 2.0 ** -40).all()
    # w8_linear on CPU tensors is the reference path; `out` is filled in place
    out = torch.zeros(M, N, dtype=dtype)
    assert w8.w8_linear(x, q, b, act, out=out) is out and torch.equal(out, got)


SMALL = {"gpt-j-6b": dict(n_embd=64, n_layer=2, n_head=4, rotary_dim=8, n_positions=64),
         "bloom-560m": dict(hidden_size=64, n_layer=2, n_head=4)}


def _tiny(preset, vocab=97):
    cfg = dict(PRESETS_HF[preset])
    cfg.update(SMALL[preset])
    cfg.update(vocab_size=vocab)
    m = build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)
    with torch.no_grad():  # grid weights: FP8 is lossless, prefill (full precision) and decode agree
        for blk in m.h:
            for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out):
                mod.weight.copy_(w8.snap_to_grid(mod.weight))
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
def test_engine_fp8_matches_forward(preset):
    m = _tiny(preset)
    prompts = [[5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8, 9], [11, 12, 13]]
    eng = LLMEngine(m, max_slots=4, max_len=48, weight_dtype="fp8")
    r = eng.runner
    assert r._w8 is not None and len(r._w8) == 4 * len(m.h)
    reqs = eng.generate(prompts, SamplingParams(max_new_tokens=8, do_sample=False))
    assert r.w8_steps > 0 and r.batched_steps == 0 and r.fused_steps == 0
    # fp32 model, lossless weights: the two paths differ by fp32 summation order only, so any margin
    # above that noise (1e-4 on O(1) logits is 1000x it) must hold
    checked = sum(_check_against_forward(m, p, q.output, margin=1e-4) for p, q in zip(prompts, reqs))
    assert checked >= 12  # at least half of the 24 generated tokens


def test_engine_option_off_by_default_and_env(monkeypatch):
    m = _tiny("gpt-j-6b")
    monkeypatch.delenv("KCA_DECODE_WEIGHTS", raising=False)
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.runner._w8 is None
    eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))
    assert eng.runner.w8_steps == 0
    monkeypatch.setenv("KCA_DECODE_WEIGHTS", "0")
    assert LLMEngine(m, max_slots=2, max_len=32).runner._w8 is None
    monkeypatch.setenv("KCA_DECODE_WEIGHTS", "fp8")
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.runner._w8 is not None
    out = eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))[0].output
    assert eng.runner.w8_steps > 0 and len(out) == 3
    monkeypatch.setenv("KCA_DECODE_WEIGHTS", "int3")
    with pytest.raises(ValueError, match="KCA_DECODE_WEIGHTS"):
        LLMEngine(m, max_slots=2, max_len=32)
    with pytest.raises(ValueError, match="weight_dtype"):
        LLMEngine(m, max_slots=2, max_len=32, weight_dtype="fp4")


def test_engine_fp8_refuses_tp_and_layer_split():
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=64, n_layer=2, n_head=4, vocab_size=96)
    tp = emulated_rank_model(LMConfig.from_hf(cfg), 2, 0, dtype=torch.float32)
    with pytest.raises(ValueError, match="fp8.*tensor-parallel"):
        LLMEngine(tp, max_slots=2, max_len=32, weight_dtype="fp8")
    m = _tiny("gpt-j-6b")
    m.h[1].to("meta")  # a second device under the last layer: a layer-split placement
    with pytest.raises(ValueError, match="fp8.*layer-split"):
        LLMEngine(m, max_slots=2, max_len=32, weight_dtype="fp8")
