"""The FP8 KV cache on the GPU (csrc/kernels/decode_kv8.hip through ops/kv8.py and the engine).

Prep: written bytes and scales against ``quantize_rows`` (bit for bit where no rotation is involved) and
against an fp64 rotation. Attention: per element against ``kv8_attention_reference(fp64=True)`` on the same
bytes and scales, under tests/test_decode_fp16_gpu.py's bound (``_within``: two units in the last place of
the output plus four times the error of the fp32 reference). Engine: greedy tokens against the
teacher-forced reference of tests/test_kv8_cpu.py -- an fp32 CPU copy of the same model behind an FP8 KV
cache, so both sides carry the same quantization and only 16-bit arithmetic separates them.
"""
import pytest
import torch

from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops import kv8
from kubernetes_cloud_amd.ops.rope import rope_tables

from .test_decode_fp16_gpu import _within
from .test_decode_gpu import _paginate
from .test_kv8_cpu import check_against_top2, teacher_forced_top2
from .test_w8_gpu import NEW, ROUNDS, make_prompts, small_lm

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
BF16, F16 = torch.bfloat16, torch.float16
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11}  # one unit in the last place, relative to the value


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _paginate3(sc, PS, seed):
    """``_paginate`` of a scale tensor [S, Hkv, L] -> ([pages + 1, Hkv, PS], block table)."""
    pool, tbl = _paginate(sc[..., None].contiguous(), PS, seed)
    return pool[..., 0].contiguous(), tbl


# ------------------------------------------------------------------------------------------ prep
def _rotate64(rows, rot, inter, cos, sin, pos):
    """fp64 RoPE of head rows [B, n, D] at positions ``pos`` (ops/decode.py's convention)."""
    x = rows.double().clone()
    if rot == 0:
        return x
    c, s = cos.double()[pos.long()][:, None, :], sin.double()[pos.long()][:, None, :]
    xr = x[..., :rot]
    if inter:
        a, b = xr[..., 0::2], xr[..., 1::2]
        out = torch.stack((a * c - b * s, b * c + a * s), dim=-1).flatten(-2)
    else:
        a, b = xr[..., :rot // 2], xr[..., rot // 2:]
        out = torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    x[..., :rot] = out
    return x


@pytest.mark.parametrize("H,Hkv,D,rot,inter", [(4, 4, 64, 0, False), (4, 4, 256, 64, True), (8, 8, 96, 24, False),
                                               (8, 2, 128, 128, False)])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("PS", [0, 16])
def test_kv8_prep(H, Hkv, D, rot, inter, dtype, PS):
    """kca_kv8_prep at positions 0, 15 and 16 (a page boundary). V rows, and K rows without rotation, are
    ``quantize_rows`` of the input rows bit for bit. Rotated K rows against the fp64 rotation k64: the
    scale within 1 +- 2u of absmax(k64) / 448 and |dequant - k64| <= (2^-4 + 2u) |k64| + 2^-10 scale, u one
    unit in the last place of the 16-bit type (the 16-bit rounding can move a value across an e4m3
    boundary). Everything outside the written rows keeps its sentinel.

    Q: bf16 is bit-equal to what kca_decode_prep leaves. That kernel has no fp16 instantiation (the fp16
    engine rotates Q in registers inside kca_decode_prep_attn_f16), so fp16 Q is held to the correctly
    rounded fp64 rotation plus the error of an fp32 rotation: half a unit in the last place (2^-11 |q64|),
    2^-20 (|x| + |partner|) for the two fp32 products and their sum, and half the smallest subnormal."""
    g = _gen(D + rot + PS)
    B, S, L = 3, 4, 32
    u = ULP[dtype]
    qkv = (torch.randn(B, (H + 2 * Hkv) * D, generator=g, device=dev) * 2).to(dtype)
    pos = torch.tensor([0, 15, 16], device=dev, dtype=torch.int32)
    slots = torch.tensor([2, 0, 3], device=dev, dtype=torch.int32)
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    shape = (S * (L // PS) + 1, Hkv, PS, D) if PS else (S, Hkv, L, D)
    tbl = None
    if PS:
        tbl = torch.randperm(S * (L // PS), generator=torch.Generator().manual_seed(1)).view(S, L // PS)
        tbl = tbl.to(torch.int32).to(dev)
    k8 = torch.full(shape, 0x55, dtype=torch.uint8, device=dev)
    v8 = torch.full(shape, 0x55, dtype=torch.uint8, device=dev)
    ks = torch.full(shape[:-1], -3.0, device=dev)
    vs = torch.full(shape[:-1], -3.0, device=dev)
    q8 = qkv.clone()
    kv8.kv8_prep(q8, H, Hkv, D, rot, inter, cos, sin, pos, slots, k8, v8, ks, vs, tbl)
    torch.cuda.synchronize()

    rows_in = qkv.view(B, H + 2 * Hkv, D)
    # the rows the step wrote, as (page or slot, row) per sequence
    sl, p = slots.long(), pos.long()
    if PS:
        sl, p = tbl.long()[sl, p // PS], p % PS
    # V (and unrotated K): bit-equal to quantize_rows of the input rows (the contract: IEEE fp32 on the CPU)
    def same(got8, gots, rows, what):
        wq, ws_ = kv8.quantize_rows(rows.cpu())
        nb, ns = int((got8.cpu() != wq).sum()), int((gots.cpu() != ws_).sum())
        dq, ds = kv8.quantize_rows(rows)  # (torch's own GPU ops, for the record)
        print(f"{what}: {nb} bytes / {ns} scales differ from the CPU contract; torch on the GPU differs from it in "
              f"{int((dq.cpu() != wq).sum())} / {int((ds.cpu() != ws_).sum())}")
        assert nb == 0 and ns == 0, what

    same(v8[sl, :, p], vs[sl, :, p], rows_in[:, H + Hkv:], "V")
    kq_got, ks_got = k8[sl, :, p], ks[sl, :, p]
    assert not bool(((kq_got == 0x7F) | (kq_got == 0xFF)).any())
    if rot == 0:
        same(kq_got, ks_got, rows_in[:, H:H + Hkv], "K")
    else:
        k64 = _rotate64(rows_in[:, H:H + Hkv], rot, inter, cos, sin, pos)
        want = k64.abs().amax(-1) / 448.0
        ratio = ks_got.double() / want
        print(f"scale ratio in [{ratio.min().item():.6f}, {ratio.max().item():.6f}] (bound 1 +- {2 * u:.2e})")
        assert bool(((ratio >= 1 - 2 * u) & (ratio <= 1 + 2 * u)).all())
        deq = kv8.dequantize_rows(kq_got, ks_got, torch.float64)
        err = (deq - k64).abs()
        tol = (2.0 ** -4 + 2 * u) * k64.abs() + 2.0 ** -10 * ks_got.double()[..., None]
        print(f"rotated K: worst err / bound {(err / tol).max().item():.3f}")
        assert bool((err <= tol).all())
    # sentinels everywhere else
    mask = torch.zeros(shape[:-1], dtype=torch.bool, device=dev)
    mask[sl, :, p] = True
    for c8, sc in ((k8, ks), (v8, vs)):
        assert bool((c8[~mask] == 0x55).all()) and bool((sc[~mask] == -3.0).all())
    # Q; the K / V part of the row is untouched
    assert torch.equal(q8.view(B, -1, D)[:, H:], rows_in[:, H:])
    if dtype == BF16:
        q16 = qkv.clone()
        kc = torch.zeros(shape, dtype=dtype, device=dev)
        dops.decode_prep(q16, H, Hkv, D, rot, inter, cos, sin, pos, slots, kc, torch.zeros_like(kc), tbl)
        assert torch.equal(q8, q16)
    else:
        q64 = _rotate64(rows_in[:, :H], rot, inter, cos, sin, pos)
        x = rows_in[:, :H].double().abs()
        partner = x.clone()
        if rot:
            xr = x[..., :rot]
            partner[..., :rot] = (xr.reshape(B, H, rot // 2, 2).flip(-1).reshape(B, H, rot) if inter
                                  else torch.cat((xr[..., rot // 2:], xr[..., :rot // 2]), -1))
        tol = 2.0 ** -11 * q64.abs() + 2.0 ** -20 * (x + partner) + 2.0 ** -25
        got = q8.view(B, -1, D)[:, :H].double()
        assert bool(((got - q64).abs() <= tol).all())
        assert torch.equal(q8.view(B, -1, D)[:, :H, rot:], rows_in[:, :H, rot:])


# ------------------------------------------------------------------------------------- attention
KV_LENS = [1, 257, 333]  # one token, one past the single-split limit, several splits


def _attn_case(D, G, PS, dtype, seed):
    """Byte caches for 3 sequences in slots (2, 0, 1) of 4 (+ the paged pool's scratch page), with the
    planted edges: a K row and a V row scaled by 2^10, an all-zero K / V row, and 0x7F bytes with NaN
    scales everywhere past a sequence's length, in the unused slot / pages and in the scratch page."""
    g = _gen(seed)
    Hkv, L, S = 2, 336, 4
    H = Hkv * G
    kf = torch.randn(S, Hkv, L, D, generator=g, device=dev)
    vf = torch.randn(S, Hkv, L, D, generator=g, device=dev)
    slots = torch.tensor([2, 0, 1], device=dev, dtype=torch.int32)
    kf[0, 1, 100] *= 2.0 ** 10   # sequence 1 (slot 0)
    vf[1, 0, 200] *= 2.0 ** 10   # sequence 2 (slot 1)
    kf[1, 0, 7] = 0.0
    vf[1, 0, 7] = 0.0
    vf[0, 1, 9] = 0.0
    k8, ks = kv8.quantize_rows(kf)
    v8, vs = kv8.quantize_rows(vf)
    assert float(ks[1, 0, 7]) == 1.0 and not bool(k8[1, 0, 7].any())
    used = torch.zeros(S, L, dtype=torch.bool, device=dev)
    for b, s_ in enumerate(slots.tolist()):
        used[s_, :KV_LENS[b]] = True
    dead = (~used)[:, None, :].expand(S, Hkv, L)
    for c8, sc in ((k8, ks), (v8, vs)):
        c8[dead] = 0x7F
        sc[dead] = float("nan")
    tbl = None
    if PS:
        k8, tbl = _paginate(k8, PS, 3)
        v8, _ = _paginate(v8, PS, 3)
        ks, _ = _paginate3(ks, PS, 3)
        vs, _ = _paginate3(vs, PS, 3)
        for c8, sc in ((k8, ks), (v8, vs)):  # the scratch page
            c8[-1] = 0x7F
            sc[-1] = float("nan")
    q = (torch.randn(3, (H + 2 * Hkv) * D, generator=g, device=dev)).to(dtype)
    return q, k8, v8, ks, vs, slots, tbl, H, L


def _attn_check(q, k8, v8, ks, vs, slots, lens, H, L, scale, alibi, tbl, window, chunk, ws, what):
    B, D = q.shape[0], k8.shape[3]
    refs = []
    for f64 in (True, False):
        o = torch.empty(B, H * D, device=dev, dtype=torch.float64 if f64 else torch.float32)
        refs.append(kv8.kv8_attention_reference(q, k8, v8, ks, vs, slots, lens, H, scale, alibi, o, tbl, window,
                                                fp64=f64))
    out = torch.full((B, H * D), float("nan"), device=dev, dtype=q.dtype)
    y = kv8.kv8_attention(q, k8, v8, ks, vs, slots, lens, H, L, scale, alibi, out=out, ws=ws, chunk=chunk,
                          block_table=tbl, window=window)
    y = y.clone()
    y2 = kv8.kv8_attention(q, k8, v8, ks, vs, slots, lens, H, L, scale, alibi, out=out, ws=ws, chunk=chunk,
                           block_table=tbl, window=window)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), what
    assert torch.equal(y, y2), what  # the same call twice: the same bits
    _within(y, refs[0], refs[1], what)


@pytest.mark.parametrize("D", [64, 96, 128, 256])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("window", [0, 40])
@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kv8_attention(D, G, alibi, window, PS, dtype):
    """kca_kv8_attn per element: the default ``decode_chunk`` (64-token splits at this length: six splits,
    empty ones under the 40-token window), ``chunk=64`` as the issue sets it, and -- added -- one 512-token
    split (several iterations of one workgroup); then the same workspace again with other lengths."""
    q, k8, v8, ks, vs, slots, tbl, H, L = _attn_case(D, G, PS, dtype, D + G + PS)
    lens = torch.tensor(KV_LENS, device=dev, dtype=torch.int32)
    al = (2.0 ** -torch.arange(1, H + 1, device=dev, dtype=torch.float32)) if alibi else None
    scale = D ** -0.5
    ws = torch.zeros(dops.decode_ws_floats(3, H, 2, D, L, 64) + 16, device=dev, dtype=torch.float32)
    for chunk in (0, 64, 512):
        _attn_check(q, k8, v8, ks, vs, slots, lens, H, L, scale, al, tbl, window, chunk, ws,
                    f"D={D} G={G} alibi={alibi} window={window} PS={PS} chunk={chunk}")
    # the same workspace with shorter lengths (every row read stays inside the planted live ranges)
    lens2 = torch.tensor([1, 64, 130], device=dev, dtype=torch.int32)
    _attn_check(q, k8, v8, ks, vs, slots, lens2, H, L, scale, al, tbl, window, 64, ws, "reused workspace")


def test_kv8_attention_refuses_unsupported_shapes():
    """head_dim 72 with three query heads per KV head: a nonzero status, and ``out`` is not written."""
    D, Hkv, G, L = 72, 2, 3, 64
    H = Hkv * G
    k8 = torch.zeros(2, Hkv, L, D, dtype=torch.uint8, device=dev)
    ks = torch.ones(2, Hkv, L, device=dev)
    q = torch.randn(1, H * D, device=dev).to(BF16)
    out = torch.full((1, H * D), 5.0, device=dev, dtype=BF16)
    slots = torch.zeros(1, dtype=torch.int32, device=dev)
    lens = torch.full((1,), 40, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="kca_kv8_attn returned status"):
        kv8.kv8_attention(q, k8, k8.clone(), ks, ks.clone(), slots, lens, H, L, out=out)
    D = 12  # not a multiple of 8
    k8 = torch.zeros(2, Hkv, L, D, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="kca_kv8_attn returned status"):
        kv8.kv8_attention(q[:, :2 * D], k8, k8.clone(), ks, ks.clone(), slots, lens, 2, L, out=out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert not kv8.supported(72, 6, 2) and not kv8.supported(12, 2, 2) and kv8.supported(96, 8, 2)


# ---------------------------------------------------------------------------------------- engine
# The top-2 margin above which a token is checked: 0.1 (tests/test_w8_gpu.py's value) or four times the
# largest difference of a top-2 log-prob between the reference run in fp32 and the same reference with a
# bf16 model, whichever is larger (a flip moves two logits; the factor leaves two on top). Measured on
# the CPU over each case's own prompts (make_prompts(B, 10 B + r), r < ROUNDS[B]), both runs teacher-forced
# with the fp32 run's greedy tokens; the largest difference per (preset, B):
#   gpt-j-6b     0.0260 / 0.0292 / 0.0340      gpt-neox-20b  0.0304 / 0.0329 / 0.0338
#   bloom-560m   0.0668 / 0.0709 / 0.0764      gpt2          0.0251 / 0.0326 / 0.0426     (B = 1 / 3 / 20)
# With small_lm's doubled final LayerNorm gain, the fraction of the reference's own greedy tokens that
# clear these margins was 0.52 .. 1.0 per case (lowest: gpt-neox-20b B = 20 between 0.52 and 0.65, gpt2
# B = 1 0.69, gpt-j-6b B = 3 about 0.6; bloom-560m 1.0 throughout), so the gain stays at 2.
# The long-prompt case: 0.0390 (0.625 of its 16 tokens clear 0.157). An fp16 model: 0.0078 over the B = 3
# prompts (0.004 over the long ones), so its margin is the 0.1 floor.
_DIFF = {("gpt-j-6b", 1): 0.0260, ("gpt-j-6b", 3): 0.0292, ("gpt-j-6b", 20): 0.0340,
         ("gpt-neox-20b", 1): 0.0304, ("gpt-neox-20b", 3): 0.0329, ("gpt-neox-20b", 20): 0.0338,
         ("bloom-560m", 1): 0.0668, ("bloom-560m", 3): 0.0709, ("bloom-560m", 20): 0.0764,
         ("gpt2", 1): 0.0251, ("gpt2", 3): 0.0326, ("gpt2", 20): 0.0426,
         "long": 0.0391, "fp16": 0.0079}


def _margin(key):
    return max(0.1, 4 * _DIFF[key])


def _cpu_copy(m, preset, dtype=torch.float32):
    c = small_lm(preset, dtype=dtype, device="cpu")
    c.load_state_dict({k: v.detach().to("cpu", dtype) for k, v in m.state_dict().items()})
    return c


def _greedy_rounds(eng, ref_model, B, max_len, margin):
    from kubernetes_cloud_amd.engine.llm_engine import SamplingParams
    checked = total = 0
    for r in range(ROUNDS[B]):
        prompts = make_prompts(B, 10 * B + r)
        outs = [q.output for q in eng.generate(prompts, SamplingParams(max_new_tokens=NEW, do_sample=False))]
        assert all(len(o) == NEW for o in outs)
        rows = teacher_forced_top2(ref_model, prompts, outs, max_len)
        checked += sum(check_against_top2(r_, o, margin) for r_, o in zip(rows, outs))
        total += NEW * B
    return checked, total


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [1, 3, 20])
def test_engine_kv8_decode(preset, B):
    """FP8 KV cache with HIP graphs at batch 1, 3 and 20: every greedy token whose top-2 log-prob margin in
    the teacher-forced reference (module docstring) exceeds the case's margin (above) is the reference's argmax, at least half
    of the tokens are checked, the steps ran on the FP8-KV path alone, the cache has the (D + 4) / 2D size,
    and a seeded sampled run replays bit-identically."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = small_lm(preset)
    eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, kv_dtype="fp8")
    r = eng.runner
    assert r.use_graphs and r._kv8 and r._w8 is None
    checked, total = _greedy_rounds(eng, _cpu_copy(m, preset), B, 256, _margin((preset, B)))
    assert r.kv8_steps > 0 and r.batched_steps == 0 and r.fused_steps == 0 and r.w8_steps == 0
    print(f"{preset} B={B}: {checked} of {total} tokens checked")
    assert 2 * checked >= total
    D = r.D
    ref16 = 2 * sum(t.numel() for t in r.cache.k + r.cache.v)
    assert r.cache.nbytes() * 2 * D == ref16 * (D + 4)
    prompts = make_prompts(B, 10 * B)
    sp = SamplingParams(max_new_tokens=10, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
    a = [q.output for q in eng.generate(prompts, sp)]
    b = [q.output for q in eng.generate(prompts, sp)]
    assert a == b and all(len(x) == 10 for x in a)


def test_engine_kv8_long_prompts():
    """B = 2, prompts of about 300 tokens, 8 new tokens at max_len 512: several splits and the combine
    launch, and pages allocated during decode."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = small_lm("gpt-j-6b")
    g = torch.Generator().manual_seed(5)
    prompts = [[int(x) for x in torch.randint(0, 1000, (n,), generator=g)] for n in (300, 317)]
    eng = LLMEngine(m, max_slots=2, max_len=512, use_graphs=True, kv_dtype="fp8", page_size=64)
    outs = [q.output for q in eng.generate(prompts, SamplingParams(max_new_tokens=8, do_sample=False))]
    assert all(len(o) == 8 for o in outs) and eng.runner.kv8_steps > 0
    rows = teacher_forced_top2(_cpu_copy(m, "gpt-j-6b"), prompts, outs, 512)
    checked = sum(check_against_top2(r_, o, _margin("long")) for r_, o in zip(rows, outs))
    print(f"long prompts: {checked} of 16 tokens checked")
    assert checked >= 8  # at least half, as in the other engine cases (measured: 8; the CPU reference's own run 10)


def test_engine_kv8_with_fp8_weights():
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m = small_lm("gpt-j-6b")
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, kv_dtype="fp8", weight_dtype="fp8")
    # (small_lm's projections sit on the FP8 grid: quantizing them is lossless, the reference is the same)
    checked, total = _greedy_rounds(eng, _cpu_copy(m, "gpt-j-6b"), 3, 256, _margin(("gpt-j-6b", 3)))
    r = eng.runner
    assert r.kv8_steps > 0 and r.w8_steps == r.kv8_steps and r.batched_steps == 0 and r.fused_steps == 0
    print(f"kv8 + w8: {checked} of {total} tokens checked")
    assert 2 * checked >= total


def test_engine_kv8_fp16_model():
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m = small_lm("gpt-j-6b", dtype=F16)
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, kv_dtype="fp8")
    checked, total = _greedy_rounds(eng, _cpu_copy(m, "gpt-j-6b"), 3, 256, _margin("fp16"))
    assert eng.runner.kv8_steps > 0 and eng.runner.batched_steps == 0 and eng.runner.fused_steps == 0
    print(f"fp16: {checked} of {total} tokens checked")
    assert 2 * checked >= total


def test_engine_kv8_beams_paged_equal_contiguous():
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m = small_lm("gpt-neox-20b")
    prompt = make_prompts(3, 30)[2]
    beams = [LLMEngine(m, max_slots=4, max_len=256, page_size=ps, kv_dtype="fp8").beam_generate(
        prompt, num_beams=4, max_new_tokens=16, n_return=4).sequences for ps in (0, 16)]
    assert beams[0] == beams[1] and len(beams[0]) == 4
