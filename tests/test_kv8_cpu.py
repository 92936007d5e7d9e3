"""The FP8 KV cache's CPU contract (ops/kv8.py): the row quantizer, the prep / attention references,
``KVCache(kv_dtype="fp8")`` and the engine option on small CPU models.

``teacher_forced_top2`` is the reference of the engine tests here and in tests/test_kv8_gpu.py: the same
model in a CPU ``ModelRunner(kv_dtype="fp8")`` -- so it carries the same quantization -- prefilled with
the prompts, then fed the tokens under test one step at a time through ``decode_topk(k=2)``.
"""
import pytest
import torch

from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.engine.runner import KVCache, ModelRunner
from kubernetes_cloud_amd.models.causal_lm import build_model
from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops import kv8
from kubernetes_cloud_amd.ops.w8 import quantize_weight

SMALL = {"gpt-j-6b": dict(n_embd=64, n_layer=2, n_head=4, rotary_dim=8, n_positions=64),
         "bloom-560m": dict(hidden_size=64, n_layer=2, n_head=4),
         "gpt2": dict(n_embd=64, n_layer=2, n_head=4, n_positions=64)}


def tiny(preset, vocab=97):
    cfg = dict(PRESETS_HF[preset])
    cfg.update(SMALL[preset])
    cfg.update(vocab_size=vocab)
    return build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)


# ------------------------------------------------------------------------------------- reference
def teacher_forced_top2(m, prompts, outs, max_len, page_size=0):
    """Per sequence, per generated position: (top-2 log-probs, top-2 ids) of model ``m`` (on the CPU)
    behind an FP8 KV cache, teacher-forced with ``outs``. Row i of sequence s predicts outs[s][i]."""
    B, n_new = len(prompts), len(outs[0])
    assert all(len(o) == n_new for o in outs)
    r = ModelRunner(m, max_slots=B, max_len=max_len, page_size=page_size, kv_dtype="fp8")
    T = max(len(p) for p in prompts)
    ids = torch.zeros(B, T, dtype=torch.long)
    for i, p in enumerate(prompts):
        ids[i, :len(p)] = torch.tensor(p)
    slots = list(range(B))
    lp = torch.log_softmax(r.prefill(ids, slots, [len(p) for p in prompts]).float(), -1)
    steps = [lp.topk(2)]
    for i in range(n_new - 1):
        steps.append(r.decode_topk([o[i] for o in outs], [len(p) + i for p in prompts], slots, 2))
    assert r.kv8_steps == n_new - 1
    return [[(st[0][s].cpu(), st[1][s].cpu()) for st in steps] for s in range(B)]


def check_against_top2(rows, out, margin):
    """Every token of ``out`` whose reference top-2 log-prob margin exceeds ``margin`` is the reference's
    argmax; returns how many tokens were checked."""
    n = 0
    for i, ((lp, ids), t) in enumerate(zip(rows, out)):
        if float(lp[0] - lp[1]) > margin:
            assert int(ids[0]) == t, (i, t, ids.tolist(), lp.tolist())
            n += 1
    return n


# ------------------------------------------------------------------------------------- quantizer
def test_quantize_rows_is_quantize_weight_on_rows():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 7, 32, generator=g) * torch.exp2(torch.randint(-12, 12, (3, 5, 7, 1), generator=g).float())
    x[0, 0, 0] = 0.0                       # an all-zero row
    x[1, 2, 3, 4] = float("nan")           # non-finite inputs count as 0
    x[1, 2, 4, 5] = float("inf")
    x[2, 4, 6, :] = torch.linspace(-1, 1, 32) * 2.0 ** -9 * 3  # a row with values in the subnormal range of its scale
    x[2, 4, 6, 0] = 7.0
    for xx in (x, x.to(torch.bfloat16), x.to(torch.float16)):
        q, s = kv8.quantize_rows(xx)
        assert q.dtype == torch.uint8 and q.shape == xx.shape and s.dtype == torch.float32 and s.shape == xx.shape[:-1]
        w = quantize_weight(xx.reshape(-1, 32))
        assert torch.equal(q.reshape(-1, 32), w.q) and torch.equal(s.reshape(-1), w.scale)
        assert not bool(((q == 0x7F) | (q == 0xFF)).any())
        assert float(s[0, 0, 0]) == 1.0 and not bool(q[0, 0, 0].any())
        xf = torch.nan_to_num(xx.float(), nan=0.0, posinf=0.0, neginf=0.0)
        err = (kv8.dequantize_rows(q, s) - xf).abs()
        # half a step of 3 mantissa bits, plus half the subnormal step (2^-9) of the row's scale
        assert bool((err <= 2.0 ** -4 * xf.abs() + 2.0 ** -10 * s[..., None]).all())
        assert kv8.dequantize_rows(q, s, torch.bfloat16).dtype == torch.bfloat16


# ------------------------------------------------------------------------------------ references
def _paginate(c, PS, perm):
    """Contiguous [S, Hkv, L, ...] -> shuffled page pool [S*L/PS + 1, Hkv, PS, ...]."""
    S, Hkv, L = c.shape[:3]
    nb = L // PS
    pool = torch.zeros((S * nb + 1, Hkv, PS) + tuple(c.shape[3:]), dtype=c.dtype)
    pages = c.reshape((S, Hkv, nb, PS) + tuple(c.shape[3:])).transpose(1, 2).reshape((S * nb, Hkv, PS) + tuple(c.shape[3:]))
    pool[perm] = pages
    return pool


@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("alibi,window", [(False, 0), (True, 0), (True, 10), (False, 40)])
def test_attention_reference_is_the_16bit_reference_on_the_dequantized_cache(PS, alibi, window):
    g = torch.Generator().manual_seed(PS + window)
    S, Hkv, G, L, D = 3, 2, 2, 64, 16
    H = Hkv * G
    k8, ks = kv8.quantize_rows(torch.randn(S, Hkv, L, D, generator=g))
    v8, vs = kv8.quantize_rows(torch.randn(S, Hkv, L, D, generator=g) * 3)
    slots = torch.tensor([2, 0], dtype=torch.int32)
    lens = torch.tensor([37, 64], dtype=torch.int32)
    for b, s_ in enumerate(slots.tolist()):  # everything past a sequence's length: NaN bytes, NaN scales
        n = int(lens[b])
        k8[s_, :, n:], v8[s_, :, n:] = 0x7F, 0x7F
        ks[s_, :, n:], vs[s_, :, n:] = float("nan"), float("nan")
    tbl = None
    if PS:
        perm = torch.randperm(S * (L // PS), generator=g)
        k8, v8, ks, vs = (_paginate(t, PS, perm) for t in (k8, v8, ks, vs))
        tbl = perm.view(S, L // PS).to(torch.int32)
    q = torch.randn(2, H * D, generator=g)
    al = torch.tensor([0.5, 0.25, 0.125, 0.0625]) if alibi else None
    y = kv8.kv8_attention_reference(q, k8, v8, ks, vs, slots, lens, H, 0.25, al, block_table=tbl, window=window)
    kd, vd = kv8.dequantize_rows(k8, ks), kv8.dequantize_rows(v8, vs)
    ref = dops.decode_attention_reference(q, kd, vd, slots, lens, H, 0.25, al, block_table=tbl, window=window)
    assert bool(torch.isfinite(y).all()) and torch.equal(y, ref)
    y64 = kv8.kv8_attention_reference(q, k8, v8, ks, vs, slots, lens, H, 0.25, al, block_table=tbl, window=window,
                                      fp64=True)
    assert y64.dtype == q.dtype and torch.allclose(y64, y, atol=1e-5, rtol=1e-5)
    # the dispatching wrapper on CPU tensors is the reference
    assert torch.equal(kv8.kv8_attention(q, k8, v8, ks, vs, slots, lens, H, L, 0.25, al, block_table=tbl,
                                         window=window), y)


@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("rot,inter", [(0, False), (8, True), (16, False)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_prep_reference_quantizes_what_decode_prep_writes(PS, rot, inter, dtype):
    g = torch.Generator().manual_seed(rot + PS)
    S, H, Hkv, L, D, B = 4, 4, 2, 32, 16, 3
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).to(dtype)
    pos = torch.tensor([0, 15, 16], dtype=torch.int32)
    slots = torch.tensor([2, 0, 3], dtype=torch.int32)
    cos, sin = (torch.randn(L, rot // 2, generator=g), torch.randn(L, rot // 2, generator=g)) if rot else (None, None)
    shape = (S * (L // PS) + 1, Hkv, PS, D) if PS else (S, Hkv, L, D)
    tbl = torch.randperm(S * (L // PS), generator=g).view(S, L // PS).to(torch.int32) if PS else None
    k16, v16 = torch.full(shape, 7.0, dtype=dtype), torch.full(shape, 7.0, dtype=dtype)
    q16 = qkv.clone()
    dops.decode_prep(q16, H, Hkv, D, rot, inter, cos, sin, pos, slots, k16, v16, tbl)
    k8, v8 = torch.full(shape, 0x55, dtype=torch.uint8), torch.full(shape, 0x55, dtype=torch.uint8)
    ks, vs = torch.full(shape[:-1], -3.0), torch.full(shape[:-1], -3.0)
    q8 = qkv.clone()
    kv8.kv8_prep(q8, H, Hkv, D, rot, inter, cos, sin, pos, slots, k8, v8, ks, vs, tbl)
    assert torch.equal(q8, q16)  # Q rotated in place exactly as today
    written = k16 != 7.0
    rows = written.any(-1)
    assert int(rows.sum()) == B * Hkv
    for c16, c8, sc in ((k16, k8, ks), (v16, v8, vs)):
        qq, ss = kv8.quantize_rows(c16)
        assert torch.equal(c8[rows], qq[rows]) and torch.equal(sc[rows], ss[rows])
        assert bool((c8[~rows] == 0x55).all()) and bool((sc[~rows] == -3.0).all())


# ----------------------------------------------------------------------------------------- cache
@pytest.mark.parametrize("D", [64, 96, 128, 256])
@pytest.mark.parametrize("page", [0, 16])
def test_cache_bytes(D, page):
    a = KVCache(2, 3, 2, 64, D, "cpu", torch.bfloat16, page_size=page)
    b = KVCache(2, 3, 2, 64, D, "cpu", torch.bfloat16, page_size=page, kv_dtype="fp8")
    assert a.k[0].dtype == torch.bfloat16 and a.k_scale is None and a.v_scale is None  # the default is unchanged
    assert b.k[0].dtype == torch.uint8 and b.k[0].shape == a.k[0].shape and b.v[1].shape == a.v[1].shape
    assert b.k_scale[0].dtype == torch.float32 and b.k_scale[0].shape == a.k[0].shape[:-1]
    assert b.nbytes() * 2 * D == a.nbytes() * (D + 4)
    with pytest.raises(ValueError, match="int4"):
        KVCache(2, 3, 2, 64, D, "cpu", torch.bfloat16, kv_dtype="int4")


def _fill(cache, g):
    for li in range(len(cache.k)):
        cache.k[li].copy_(torch.randint(0, 0x7F, cache.k[li].shape, generator=g).to(torch.uint8))
        cache.v[li].copy_(torch.randint(0, 0x7F, cache.v[li].shape, generator=g).to(torch.uint8))
        cache.k_scale[li].copy_(torch.rand(cache.k_scale[li].shape, generator=g))
        cache.v_scale[li].copy_(torch.rand(cache.v_scale[li].shape, generator=g))


@pytest.mark.parametrize("page", [0, 16])
def test_cache_fork_copies_bytes_and_scales(page):
    g = torch.Generator().manual_seed(page)
    c = KVCache(2, 4, 2, 64, 8, "cpu", torch.bfloat16, page_size=page, kv_dtype="fp8")
    upto = 37  # two full pages and a partial tail page of 5 rows
    c.reserve(0, upto)
    _fill(c, g)
    c.fork([1, 2], [0, 0], upto)
    for li in range(2):
        for t, sc in ((c.k[li], c.k_scale[li]), (c.v[li], c.v_scale[li])):
            src = dops.gather_kv(t, 0, upto, c.table_h if page else None)
            src_s = dops.gather_kv(sc[..., None], 0, upto, c.table_h if page else None)
            for d in (1, 2):
                assert torch.equal(dops.gather_kv(t, d, upto, c.table_h if page else None), src)
                assert torch.equal(dops.gather_kv(sc[..., None], d, upto, c.table_h if page else None), src_s)
    if page:  # full pages shared, the tail page a copy of its own
        assert c.pages[1][:2] == c.pages[0][:2] and c.pages[1][2] not in (c.pages[0][2], c.pages[2][2])


# ---------------------------------------------------------------------------------------- engine
PROMPTS = [[5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19], [11, 12, 13, 14, 15]]


@pytest.mark.parametrize("preset", list(SMALL))
def test_engine_greedy_paged_equals_contiguous(preset):
    m = tiny(preset)
    sp = SamplingParams(max_new_tokens=10, do_sample=False)
    outs = {}
    for page in (0, 16):
        eng = LLMEngine(m, max_slots=4, max_len=48, page_size=page, kv_dtype="fp8")
        r = eng.runner
        assert r._kv8 and r.cache.k[0].dtype == torch.uint8
        outs[page] = [q.output for q in eng.generate(PROMPTS, sp)]
        assert r.kv8_steps > 0 and r.fused_steps == 0 and r.batched_steps == 0 and r.w8_steps == 0
    assert outs[0] == outs[16] and all(len(o) == 10 for o in outs[0])
    # the engine's tokens are the teacher-forced reference's argmax wherever its margin is clear: both are
    # the same fp32 arithmetic on the same quantized cache up to summation order (1e-4 is 1000x that)
    rows = teacher_forced_top2(m, PROMPTS, outs[0], 48)
    assert sum(check_against_top2(r_, o, 1e-4) for r_, o in zip(rows, outs[0])) >= 15


def test_engine_with_fp8_weights_too():
    m = tiny("gpt-j-6b")
    eng = LLMEngine(m, max_slots=4, max_len=48, kv_dtype="fp8", weight_dtype="fp8")
    out = eng.generate(PROMPTS, SamplingParams(max_new_tokens=6, do_sample=False))
    r = eng.runner
    assert all(len(q.output) == 6 for q in out)
    assert r.kv8_steps > 0 and r.w8_steps == r.kv8_steps and r.fused_steps == 0 and r.batched_steps == 0


def test_beam_search_paged_equals_contiguous():
    m = tiny("gpt-j-6b")
    prompt = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2]
    res = {}
    for page in (0, 16):
        eng = LLMEngine(m, max_slots=4, max_len=64, page_size=page, kv_dtype="fp8")
        res[page] = eng.beam_generate(prompt, num_beams=3, max_new_tokens=12, n_return=3)
        assert eng.runner.kv8_steps > 0
        if page:
            assert eng.runner.cache.free_count() == eng.runner.cache.n_pages
    assert res[0].sequences == res[16].sequences and len(res[0].sequences) == 3


@pytest.mark.parametrize("preset,page", [("gpt-j-6b", 16), ("bloom-560m", 0)])
def test_chunked_prefill(preset, page):
    """A long prompt prefilled in chunks of <= 8 tokens while another stream decodes. A chunk sees the
    earlier chunks as stored (quantized) and itself exact, the reference's one-pass prefill sees the whole
    prompt exact, so the two differ by the quantization noise of the prefix: e4m3 rows carry a relative
    error of up to 2^-4 per element, which the issue behind this mode measured as up to 0.15 on a logit
    of a shrunk model; a flip moves two logits, so tokens are compared where the reference's top-2
    margin exceeds 0.3."""
    m = tiny(preset)
    g = torch.Generator().manual_seed(3)
    short = torch.randint(0, 97, (5,), generator=g).tolist()
    long = torch.randint(0, 97, (45,), generator=g).tolist()
    eng = LLMEngine(m, max_slots=4, max_len=64, page_size=page, prefill_chunk=8, kv_dtype="fp8")
    r1 = eng.add_request(short, SamplingParams(max_new_tokens=14, do_sample=False))
    eng.step()
    eng.step()
    r2 = eng.add_request(long, SamplingParams(max_new_tokens=6, do_sample=False))
    eng.run_until_done([r1, r2])
    assert eng.stats["prefill_chunks"] >= 5 and len(r1.output) == 14 and len(r2.output) == 6
    assert eng.runner.kv8_steps > 0
    n = 0
    for p, o in ((short, r1.output), (long, r2.output)):
        n += check_against_top2(teacher_forced_top2(m, [p], [o], 64, page)[0], o, 0.3)
    print(f"{preset}: {n} of 20 tokens clear the 0.3 margin")


def test_option_values(monkeypatch):
    m = tiny("gpt-j-6b")
    monkeypatch.delenv("KCA_DECODE_KV", raising=False)
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert not eng.runner._kv8 and eng.runner.cache.k[0].dtype == torch.float32 and eng.runner.cache.k_scale is None
    eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))
    assert eng.runner.kv8_steps == 0
    for off in ("0", "none", "off", ""):
        monkeypatch.setenv("KCA_DECODE_KV", off)
        assert not LLMEngine(m, max_slots=2, max_len=32).runner._kv8
    monkeypatch.setenv("KCA_DECODE_KV", "fp8")
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.runner._kv8
    assert len(eng.generate([[1, 2, 3]], SamplingParams(max_new_tokens=3, do_sample=False))[0].output) == 3
    assert eng.runner.kv8_steps > 0
    monkeypatch.setenv("KCA_DECODE_KV", "int4")
    with pytest.raises(ValueError, match="KCA_DECODE_KV.*int4"):
        LLMEngine(m, max_slots=2, max_len=32)
    monkeypatch.delenv("KCA_DECODE_KV")
    with pytest.raises(ValueError, match="kv_dtype.*e5m2"):
        LLMEngine(m, max_slots=2, max_len=32, kv_dtype="e5m2")
    with pytest.raises(ValueError, match="kv_dtype.*e5m2"):
        ModelRunner(m, max_slots=2, max_len=32, kv_dtype="e5m2")
    runner = ModelRunner(m, max_slots=2, max_len=32, kv_dtype="fp8")
    assert LLMEngine(m, runner=runner).runner._kv8
    with pytest.raises(ValueError, match="kv_dtype.*runner"):
        LLMEngine(m, runner=runner, kv_dtype="fp8")


def test_refuses_tp_layer_split_and_head_dims():
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=64, n_layer=2, n_head=4, vocab_size=96)
    tp = emulated_rank_model(LMConfig.from_hf(cfg), 2, 0, dtype=torch.float32)
    with pytest.raises(ValueError, match="fp8.*tensor-parallel"):
        LLMEngine(tp, max_slots=2, max_len=32, kv_dtype="fp8")
    m = tiny("gpt-j-6b")
    m.h[1].to("meta")  # a second device under the last layer: a layer-split placement
    with pytest.raises(ValueError, match="fp8.*layer-split"):
        LLMEngine(m, max_slots=2, max_len=32, kv_dtype="fp8")
    cfg = dict(PRESETS_HF["gpt2"])
    cfg.update(n_embd=48, n_layer=1, n_head=4, n_positions=32, vocab_size=50)  # head_dim 12
    odd = build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)
    with pytest.raises(ValueError, match="fp8.*head_dim 12"):
        LLMEngine(odd, max_slots=2, max_len=32, kv_dtype="fp8")
