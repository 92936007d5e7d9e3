"""``LLMEngine(weight_dtype=..., prefill_weights="quantized")`` on the GPU: prefill through ``kca_wq_gemm``
on the quantized weights, the 16-bit projection weights released.

The served model can no longer run its own forward, so greedy tokens are compared with the forward of a
second ``small_lm(preset)`` -- the same seed, hence the same bytes -- through ``check_against_forward`` at
margin 0.1, and at least ONE THIRD of the generated tokens must clear the margin, for both formats: fp32
CPU forwards of these presets on prompts of 70 to 199 tokens cleared it for 0.48 .. 1.00 of their tokens
with MXFP4-snapped weights and for 0.56 .. 1.00 with FP8-snapped ones (four runs of 48 tokens per preset),
so the FP8 tests' one-half would sit too close to 0.56.
"""
import gc

import pytest
import torch

from kubernetes_cloud_amd.ops import mx4, w8

from . import test_mx4_gpu as tm
from . import test_w8_gpu as t8
from .test_w8_gpu import NEW, ROUNDS, check_against_forward

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
SMALL_LM = {"fp8": t8.small_lm, "mxfp4": tm.small_lm}
_twins: dict = {}


def _twin(fmt, preset, dtype=torch.bfloat16):
    """The reference model of a case: built once, shared, never handed to a runner."""
    key = (fmt, preset, dtype)
    if key not in _twins:
        _twins[key] = SMALL_LM[fmt](preset, dtype=dtype)
    return _twins[key]


def long_prompts(B, seed):
    """70 to 199 random tokens: every prompt prefills with M > 64 (``make_prompts`` gives 8 to 89)."""
    g = torch.Generator().manual_seed(seed)
    return [[int(x) for x in torch.randint(0, 1000, (int(n),), generator=g)]
            for n in torch.randint(70, 200, (B,), generator=g)]


def _decode_counters_ok(r, fmt):
    if fmt == "fp8":
        return r.w8_steps > 0 and r.mx4_steps == 0 and r.batched_steps == 0 and r.fused_steps == 0
    return tm._only_mx4_steps(r)


def _greedy_rounds(eng, twin, B):
    from kubernetes_cloud_amd.engine.llm_engine import SamplingParams
    checked = total = 0
    for r in range(ROUNDS[B]):
        prompts = long_prompts(B, 10 * B + r)
        outs = [q.output for q in eng.generate(prompts, SamplingParams(max_new_tokens=NEW, do_sample=False))]
        assert all(len(o) == NEW for o in outs)
        checked += sum(check_against_forward(twin, p, o) for p, o in zip(prompts, outs))
        total += NEW * B
    return checked, total


def _released(m):
    return all(mod.weight.numel() == 0 and mod.weight.dtype == next(m.parameters()).dtype
               for blk in m.h for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out))


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_engine_quantized_prefill(fmt, B, preset, monkeypatch):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m, twin = SMALL_LM[fmt](preset), _twin(fmt, preset)
    calls = tm._spy(monkeypatch)
    eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, weight_dtype=fmt, prefill_weights="quantized")
    r = eng.runner
    assert r.use_graphs and r._wq_prefill and _released(m)
    with pytest.raises(RuntimeError, match='prefill_weights="quantized"'):
        m.h[0].mlp.fc_in(torch.zeros(1, m.cfg.hidden, device=dev, dtype=torch.bfloat16))
    # the quantized weights reproduce the twin's snapped ones
    deq = (w8 if fmt == "fp8" else mx4).dequantize
    qs = r._w8 if fmt == "fp8" else r._mx4
    assert torch.equal(deq(qs[id(m.h[0].mlp.fc_out)], torch.bfloat16), twin.h[0].mlp.fc_out.weight)
    checked, total = _greedy_rounds(eng, twin, B)
    assert ("kca_wq_gemm", 0) in calls and all(rc == 0 for name, rc in calls if name == "kca_wq_gemm")
    assert r.wq_prefill_steps > 0 and r.wq_prefill_steps % (4 * len(m.h)) == 0
    assert _decode_counters_ok(r, fmt)
    print(f"{fmt} {preset} B={B}: {checked} of {total} tokens checked")
    assert 3 * checked >= total
    prompts = long_prompts(B, 10 * B)
    sp = SamplingParams(max_new_tokens=10, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
    a = [q.output for q in eng.generate(prompts, sp)]
    b = [q.output for q in eng.generate(prompts, sp)]
    assert a == b and all(len(x) == 10 for x in a)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_engine_quantized_prefill_fp16_model(fmt, monkeypatch):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m, twin = SMALL_LM[fmt]("gpt-j-6b", dtype=torch.float16), _twin(fmt, "gpt-j-6b", torch.float16)
    calls = tm._spy(monkeypatch)
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype=fmt, prefill_weights="quantized")
    checked, total = _greedy_rounds(eng, twin, 3)
    assert ("kca_wq_gemm", 0) in calls and eng.runner.wq_prefill_steps > 0 and _decode_counters_ok(eng.runner, fmt)
    print(f"{fmt} fp16: {checked} of {total} tokens checked")
    assert 3 * checked >= total


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_engine_quantized_prefill_chunked(fmt):
    """``prefill_chunk=64``: a long prompt admitted while another request decodes is prefilled in chunks
    (``start=``, ``_continued_attention``) between the decode steps of the running one; both outputs pass the
    forward check."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m, twin = SMALL_LM[fmt]("gpt-neox-20b"), _twin(fmt, "gpt-neox-20b")
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype=fmt, prefill_weights="quantized",
                    prefill_chunk=64)
    first, second = long_prompts(2, 77)
    sp = SamplingParams(max_new_tokens=NEW, do_sample=False)
    r1 = eng.add_request(first, sp)
    eng.step()
    eng.step()
    assert len(r1.output) >= 1
    r2 = eng.add_request(second, sp)
    eng.run_until_done([r1, r2])
    assert eng.stats["prefill_chunks"] >= 2 and eng.runner.wq_prefill_steps > 0
    assert len(r1.output) == NEW and len(r2.output) == NEW
    checked = check_against_forward(twin, first, r1.output) + check_against_forward(twin, second, r2.output)
    print(f"{fmt} chunked: {checked} of {2 * NEW} tokens checked")
    assert 3 * checked >= 2 * NEW


def test_engine_quantized_prefill_with_fp8_kv(monkeypatch):
    """With ``kv_dtype="fp8"``, checked as ``test_engine_mxfp4_with_fp8_kv`` checks it: against a CPU fp32
    copy of the model behind an FP8 KV cache, teacher-forced with the tokens under test. The copy is made
    from the twin (the served model's projections are empty). Margin: the larger of that test's for this
    preset and batch and the FP8-KV tests' long-prompt margin, since these prompts are long."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams

    from .test_kv8_gpu import _cpu_copy, _margin, check_against_top2, teacher_forced_top2
    m, twin = tm.small_lm("gpt-j-6b"), _twin("mxfp4", "gpt-j-6b")
    calls = tm._spy(monkeypatch)
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype="mxfp4", kv_dtype="fp8",
                    prefill_weights="quantized")
    ref = _cpu_copy(twin, "gpt-j-6b")
    margin = max(_margin(("gpt-j-6b", 3)), _margin("long"))
    checked = total = 0
    for rnd in range(ROUNDS[3]):
        prompts = long_prompts(3, 30 + rnd)
        outs = [q.output for q in eng.generate(prompts, SamplingParams(max_new_tokens=NEW, do_sample=False))]
        rows = teacher_forced_top2(ref, prompts, outs, 256)
        checked += sum(check_against_top2(r_, o, margin) for r_, o in zip(rows, outs))
        total += NEW * 3
    r = eng.runner
    assert ("kca_wq_gemm", 0) in calls and r.wq_prefill_steps > 0
    assert tm._only_mx4_steps(r) and r.kv8_steps == r.mx4_steps
    print(f"quantized prefill + mxfp4 + kv8: {checked} of {total} tokens checked")
    assert 3 * checked >= total


def test_engine_quantized_prefill_with_spec_tokens(monkeypatch):
    """With ``spec_tokens=2``: drafts scripted from the spec-off engine's outputs (every fifth one wrong, as
    in tests/test_spec_gpu.py); the outputs pass the same forward check and verify steps ran."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams

    from .test_spec_gpu import EveryFifthWrong
    twin = _twin("fp8", "gpt-neox-20b")
    sp = SamplingParams(max_new_tokens=NEW, do_sample=False)
    prompts = long_prompts(3, 41)
    kw = dict(max_slots=4, max_len=256, use_graphs=True, weight_dtype="fp8", prefill_weights="quantized")
    base = [q.output for q in LLMEngine(t8.small_lm("gpt-neox-20b"), **kw).generate(prompts, sp)]
    script = EveryFifthWrong({tuple(p): o for p, o in zip(prompts, base)})
    calls = tm._spy(monkeypatch)
    eng = LLMEngine(t8.small_lm("gpt-neox-20b"), spec_tokens=2, proposer=script, **kw)
    outs = [q.output for q in eng.generate(prompts, sp)]
    assert all(len(o) == NEW for o in outs)
    checked = sum(check_against_forward(twin, p, o) for p, o in zip(prompts, outs))
    st = eng.stats
    print(f"quantized prefill + spec: {checked} of {3 * NEW} tokens checked, {st['spec_steps']} verify steps, "
          f"{st['spec_accepted']} of {st['spec_drafted']} drafts accepted, identical to spec-off: {outs == base}")
    assert 3 * checked >= 3 * NEW
    assert ("kca_wq_gemm", 0) in calls and eng.runner.wq_prefill_steps > 0
    assert st["spec_steps"] > 0 and st["spec_accepted"] >= 1 and eng.runner.spec_steps > 0


def _build(fmt, preset, option, host=False):
    """(allocated bytes of model + runner, runner, model), the model built inside the measurement."""
    from kubernetes_cloud_amd.engine.runner import ModelRunner
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    m = SMALL_LM[fmt](preset)
    if host:
        for blk in m.h:
            for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out):
                mod.weight.data = mod.weight.data.cpu()
    r = ModelRunner(m, max_slots=2, max_len=256, use_graphs=True, weight_dtype=fmt,
                    prefill_weights="quantized" if option else None)
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - base, r, m


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_quantized_prefill_memory(fmt):
    """Two runners with identical arguments on twin models: the option's holds less device memory by the
    released bytes, within 64 KiB (no workspace on the new path; 512-byte allocator rounding over a few
    dozen tensors). The option's runner is built first, so one-time allocations of a first runner count
    against it, not for it."""
    with_opt, r1, m1 = _build(fmt, "gpt-neox-20b", True)
    wb = r1.weight_bytes()
    del r1, m1
    without, r0, m0 = _build(fmt, "gpt-neox-20b", False)
    wb0 = r0.weight_bytes()
    print(f"{fmt}: {without} B without, {with_opt} B with the option; {wb}")
    assert wb0["released_16bit"] == 0 and wb0["quantized"] == wb["quantized"] > 0
    assert wb["released_16bit"] == sum(p.numel() * 2 for blk in m0.h for p in
                                      (blk.attn.qkv.weight, blk.attn.out.weight, blk.mlp.fc_in.weight,
                                       blk.mlp.fc_out.weight))
    assert wb["resident_16bit"] == wb0["resident_16bit"] - wb["released_16bit"]
    assert without - with_opt >= wb["released_16bit"] - 64 * 1024


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_quantized_prefill_host_resident_weights(fmt):
    """Projection weights on the host when the runner is built: the same quantized bytes and the same
    greedy tokens as the all-device build."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    _, ra, ma = _build(fmt, "bloom-560m", True)
    _, rb, mb = _build(fmt, "bloom-560m", True, host=True)
    qa, qb = (ra._w8, rb._w8) if fmt == "fp8" else (ra._mx4, rb._mx4)
    for moda, modb in zip(ma.modules(), mb.modules()):
        if id(moda) in qa:
            assert qb[id(modb)].q.is_cuda and qb[id(modb)].scale.is_cuda
            assert torch.equal(qa[id(moda)].q, qb[id(modb)].q) and torch.equal(qa[id(moda)].scale, qb[id(modb)].scale)
    assert len(qb) == 4 * len(mb.h) and ra.weight_bytes() == rb.weight_bytes()
    prompts = long_prompts(2, 5)
    sp = SamplingParams(max_new_tokens=NEW, do_sample=False)
    a = [q.output for q in LLMEngine(ma, runner=ra).generate(prompts, sp)]
    b = [q.output for q in LLMEngine(mb, runner=rb).generate(prompts, sp)]
    assert a == b and all(len(o) == NEW for o in a)
