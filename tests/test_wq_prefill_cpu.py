"""``prefill_weights="quantized"`` on the CPU (engine/runner.py): fp32 models, so ``wq_linear`` takes the
reference functions and the runner logic is what is under test -- releasing the 16-bit weights, the
refusal of a direct call, the memory report, prefill and chunked prefill on the quantized weights, the
option's values.

Logit tolerance: the served model and its twin hold the same snapped weights, so dequantized weights
equal the twin's exactly and the two prefills differ by fp32 summation order only (the reference forms
``(x q^T) * scale`` / a scaled-value matmul where the twin runs ``F.linear``): |diff| <= 2e-4 + 1e-4 |ref|
on logits of magnitude ~1..10 is hundreds of fp32 units in the last place through three layers of sums of
up to 4096 terms, and four orders of magnitude below what a wrong weight, bias or activation would move.
"""
import pytest
import torch

from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.engine.runner import ModelRunner

from . import test_mx4_gpu, test_w8_gpu

CPU = torch.device("cpu")
SMALL_LM = {"fp8": test_w8_gpu.small_lm, "mxfp4": test_mx4_gpu.small_lm}
# (parallel and sequential residual, rotary / ALiBi / learned positions; the 1024-wide GPT-J preset with its
# 50400-row head takes twice as long on the CPU and adds no layer kind)
CASES = [("fp8", "gpt-neox-20b"), ("fp8", "bloom-560m"), ("mxfp4", "gpt-neox-20b"), ("mxfp4", "gpt2")]
_models: dict = {}


def _lm(fmt, preset):
    """A fresh served model (the runner empties it) and ONE shared twin per case, left unchanged."""
    key = (fmt, preset)
    if key not in _models:
        _models[key] = SMALL_LM[fmt](preset, dtype=torch.float32, device=CPU)
    return SMALL_LM[fmt](preset, dtype=torch.float32, device=CPU), _models[key]


def _projections(m):
    return [mod for blk in m.h for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out)]


def _close(got, ref, what):
    err = (got.double() - ref.double()).abs()
    tol = 2e-4 + 1e-4 * ref.double().abs()
    print(f"{what}: max |diff| {err.max().item():.3e}, worst diff/tol {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), what


@pytest.mark.parametrize("fmt,preset", CASES)
def test_quantized_prefill_releases_weights_and_matches_the_twin(fmt, preset):
    m, twin = _lm(fmt, preset)
    shapes = [tuple(mod.weight.shape) for mod in _projections(m)]
    total = sum(p.numel() * p.element_size() for p in m.parameters())
    r = ModelRunner(m, max_slots=2, max_len=128, weight_dtype=fmt, prefill_weights="quantized")
    qs = r._w8 if fmt == "fp8" else r._mx4
    assert qs is not None and len(qs) == 4 * len(m.h)
    for mod, shape in zip(_projections(m), shapes):
        assert mod.weight.numel() == 0 and mod.weight.dtype == torch.float32 and mod.weight.device == CPU
        assert r.released[id(mod)][0] == shape
        assert tuple(qs[id(mod)].shape) == shape
        assert mod.bias is None or mod.bias.numel() == shape[0]
    with pytest.raises(RuntimeError, match='prefill_weights="quantized"'):
        m.h[0].attn.qkv(torch.zeros(1, shapes[0][1]))
    with pytest.raises(RuntimeError, match='prefill_weights="quantized"'):
        m(torch.tensor([[1, 2, 3]]))
    wb = r.weight_bytes()
    assert wb["released_16bit"] == sum(a * b * 4 for a, b in shapes)
    assert wb["quantized"] == sum(q.nbytes() for q in qs.values())
    assert wb["resident_16bit"] == total - wb["released_16bit"]
    assert wb["resident_16bit"] == sum(p.numel() * p.element_size() for p in m.parameters())

    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 1000, (2, 75), generator=g)
    lens = [75, 61]
    logits = r.prefill(ids, [0, 1], lens)
    assert r.wq_prefill_steps == 4 * len(m.h)
    with torch.no_grad():
        ref = torch.stack([twin(ids[i:i + 1, :L])[0, -1] for i, L in enumerate(lens)])
    _close(logits, ref, f"{fmt} {preset} prefill")

    # the same prompt in chunks (start=): each chunk continues the slot; the last chunk's logits
    steps = r.wq_prefill_steps
    for p0, p1 in ((0, 32), (32, 40), (40, 75)):
        chunked = r.prefill(ids[:1, p0:p1], [0], [p1 - p0], start=[p0])
    assert r.wq_prefill_steps == steps + 3 * 4 * len(m.h)
    _close(chunked, logits[:1], f"{fmt} {preset} chunked prefill")


def test_chunked_engine_equals_unchunked_tokens():
    """The criterion of the existing chunked-prefill tests (tests/test_engine_cpu.py): a long prompt admitted
    while another request decodes is prefilled in chunks, and every output equals the unchunked run."""
    sp_run = SamplingParams(max_new_tokens=14, do_sample=False)
    sp_long = SamplingParams(max_new_tokens=6, do_sample=False)
    g = torch.Generator().manual_seed(3)
    short = torch.randint(0, 1000, (5,), generator=g).tolist()
    long = torch.randint(0, 1000, (90,), generator=g).tolist()
    m, _ = _lm("mxfp4", "gpt2")
    eng = LLMEngine(m, max_slots=4, max_len=128, weight_dtype="mxfp4", prefill_weights="quantized", prefill_chunk=16)
    r1 = eng.add_request(short, sp_run)
    eng.step()
    r2 = eng.add_request(long, sp_long)
    eng.run_until_done([r1, r2])
    assert eng.stats["prefill_chunks"] >= 5 and eng.runner.wq_prefill_steps > 0
    m2, _ = _lm("mxfp4", "gpt2")
    ref = LLMEngine(m2, max_slots=4, max_len=128, weight_dtype="mxfp4", prefill_weights="quantized")
    assert r2.output == ref.generate([long], sp_long)[0].output
    assert r1.output == ref.generate([short], sp_run)[0].output


def test_option_values_and_environment(monkeypatch):
    monkeypatch.delenv("KCA_PREFILL_WEIGHTS", raising=False)
    monkeypatch.delenv("KCA_DECODE_WEIGHTS", raising=False)
    m, _ = _lm("fp8", "bloom-560m")
    n_proj = 4 * len(m.h)

    def intact(model):
        return all(mod.weight.numel() > 0 for mod in _projections(model))

    with pytest.raises(ValueError, match="prefill_weights='quantized'.*needs weight_dtype"):
        ModelRunner(m, max_slots=2, max_len=64, prefill_weights="quantized")
    with pytest.raises(ValueError, match="prefill_weights='quantized'.*needs weight_dtype"):
        LLMEngine(m, max_slots=2, max_len=64, prefill_weights="quantized")
    with pytest.raises(ValueError, match="prefill_weights / KCA_PREFILL_WEIGHTS"):
        ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8", prefill_weights="int8")
    assert intact(m)
    for off in (None, "16bit", "0", "off"):
        r = ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8", prefill_weights=off)
        assert intact(m) and not r.released and r.weight_bytes()["released_16bit"] == 0
        r.prefill(torch.tensor([[1, 2, 3, 4]]), [0])
        assert r.wq_prefill_steps == 0
    m(torch.tensor([[1, 2, 3]]))  # the model still runs its own forward
    # a supplied runner sets its own
    with pytest.raises(ValueError, match="prefill_weights applies to the runner the engine builds"):
        LLMEngine(m, runner=r, prefill_weights="quantized")
    # the environment is read only when the keyword is None
    monkeypatch.setenv("KCA_PREFILL_WEIGHTS", "quantized")
    r = ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8", prefill_weights="16bit")
    assert intact(m) and not r._wq_prefill
    r = ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8", prefill_weights="off")
    assert intact(m) and not r._wq_prefill
    monkeypatch.setenv("KCA_PREFILL_WEIGHTS", "nonsense")
    assert not ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8", prefill_weights="16bit")._wq_prefill
    with pytest.raises(ValueError, match="prefill_weights / KCA_PREFILL_WEIGHTS"):
        ModelRunner(m, max_slots=2, max_len=64, weight_dtype="fp8")
    assert intact(m)
    monkeypatch.setenv("KCA_PREFILL_WEIGHTS", "quantized")
    eng = LLMEngine(m, max_slots=2, max_len=64, weight_dtype="fp8")
    assert eng.runner._wq_prefill and not intact(m) and len(eng.runner.released) == n_proj
    out = eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))[0].output
    assert len(out) == 3 and eng.runner.wq_prefill_steps == n_proj and eng.runner.w8_steps > 0
