"""FP8 weight-only decode on the GPU: ``kca_w8_gemm`` (csrc/kernels/gemv_w8.hip) per element against
fp64, and ``LLMEngine(weight_dtype="fp8")`` against the model's own forward.

Kernel bound, per element, against ``ref = act(scale[n] * sum_k x[m,k] q[n,k] + bias[n])`` computed in
fp64 from the kernel's own 16-bit x and e4m3 q:

    no activation:  |y - ref| <= u * |ref| + 2^-20 * scale[n] * sum_k |x q|
    activation:     |y - ref| <= u * |ref| + 1.13 * 2^-20 * scale[n] * sum_k |x q| + A

u = 2^-8 (bf16) / 2^-11 (fp16): half a unit in the last place of the one output rounding. The second
term is a generous fp32 accumulation error on the sum of magnitudes; 1.13 bounds |GELU'|. A is the
allowance the existing per-element GELU tests give the activation's own evaluation
(tests/test_decode_fp16_gpu.py ``_within``): four times the largest error of the same GELU evaluated in
fp32 torch on the same pre-activations, taken from the reference at run time. Inputs are scaled so
that no output lands in fp16's subnormal range, where half a unit in the last place is an absolute
2^-25 and not relative.
"""
import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd.ops import _lib, w8

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130]
NKS = [(16, 16), (272, 512), (1360, 1008), (640, 6208)]


def _spy(monkeypatch):
    """(name, status) of every entry point tried through ``_lib.call_rc``."""
    calls, real = [], _lib.call_rc

    def call_rc(name, *a):
        rc = real(name, *a)
        calls.append((name, rc))
        return rc

    monkeypatch.setattr(_lib, "call_rc", call_rc)
    return calls


def _weights(N, K, seed):
    """Quantized random rows with planted ones: row 0 all zeros, row 1 +-448, row 2 e4m3 subnormals
    (+-1..7 * 2^-9, scale 8), row 3 carrying 0x80 (-0.0) bytes."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = w8.quantize_weight(torch.randn(N, K, generator=g, device=dev) * K ** -0.5)
    k = torch.arange(K, device=dev)
    q.q[0] = 0
    q.scale[0] = 1.0
    q.q[1] = torch.where(k % 2 == 0, 0x7E, 0xFE).to(torch.uint8)
    q.scale[1] = 2.0 ** -12
    q.q[2] = ((k % 7 + 1) | torch.where(k % 3 == 0, 0x80, 0)).to(torch.uint8)
    q.scale[2] = 8.0
    q.q[3, ::5] = 0x80
    assert not ((q.q == 0x7F) | (q.q == 0xFF)).any()
    return q, g


def _act(z, act):
    return F.gelu(z, approximate="tanh") if act == 1 else F.gelu(z) if act == 2 else z


def _check(y, x, q, bias, act, what):
    """The module docstring's bound; prints the worst error / bound ratio before asserting."""
    xd, qd, sc = x.double(), q.values(torch.float64), q.scale.double()
    z = (xd @ qd.t()) * sc
    mag = (xd.abs() @ qd.abs().t()) * sc
    if bias is not None:
        z = z + bias.double()
    ref = _act(z, act)
    tol = U[y.dtype] * ref.abs() + (1.13 if act else 1.0) * 2.0 ** -20 * mag
    if act:
        tol = tol + 4 * (_act(z.float(), act).double() - ref).abs().max()
    err = (y.double() - ref).abs()
    ok = err <= tol  # (a NaN output compares False)
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}")
    assert bool(ok.all()), (what, int((~ok).sum()), err[~ok].max().item(), ratio)


def _run_case(dtype, M, N, K, monkeypatch, seed):
    q, g = _weights(N, K, seed)
    # x inside a wider buffer (ldx > K); half-scale rows keep GELU outputs out of fp16's subnormals
    xb = (torch.randn(M, K + 24, generator=g, device=dev) * 0.5).to(dtype)
    x = xb[:, :K]
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(dtype)
    calls = _spy(monkeypatch)
    launches = -(-M // w8.MAX_M)
    for act in (0, 1, 2):
        for bias in (None, b):
            for pad in (24, 13):  # row stride N + 24: 8-byte-aligned rows (packed stores); N + 13: scalar stores
                buf = torch.full((M + 2, 8 + N + pad - 8), 777.0, device=dev, dtype=dtype)
                ref_buf = buf.clone()
                out = buf[1:M + 1, 8:8 + N]
                del calls[:]
                y = w8.w8_linear(x, q, bias, act, out=out)
                assert y.data_ptr() == out.data_ptr()
                assert calls == [("kca_w8_gemm", 0)] * launches, calls  # the native kernel, one launch per slab
                what = f"w8 {dtype} M={M} N={N} K={K} act={act} bias={bias is not None} ldy=N+{pad}"
                _check(y, x, q, bias, act, what)
                # guard rows and columns of the sentinel buffer untouched
                keep = torch.ones_like(buf, dtype=torch.bool)
                keep[1:M + 1, 8:8 + N] = False
                assert torch.equal(buf[keep], ref_buf[keep]), what
                # planted rows: an all-zero weight row gives exactly 0, or the bias where nothing else rounds
                if bias is None or act == 0:
                    z0 = torch.zeros(M, device=dev, dtype=dtype) if bias is None else bias[0].expand(M)
                    assert torch.equal(y[:, 0], z0), what
                # the same call gives the same bits, with and without `out`
                y2 = w8.w8_linear(x, q, bias, act)
                assert torch.equal(y2, y), what


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_w8_gemm_per_element(dtype, N, K, M, monkeypatch):
    """Every boundary of the kernels: M = 1..4 (GEMV, row pads 1 / 2 / 4), 5..64 (MFMA, 1 / 2 / 4
    activation tiles), 65 and 130 (the 64-row slab loop); N below one wave's rows, N not a multiple of
    any workgroup tile (272 = 2 * 128 + 16, 1360 = 10 * 128 + 80), K = 16, K not a multiple of the
    128-wide chunk (1008 = 7 * 128 + 112) nor of the GEMV's 2048-wide step (6208); every activation,
    with and without bias, both store forms."""
    _run_case(dtype, M, N, K, monkeypatch, seed=M * 131 + N + K)


@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_w8_gemm_projection_shape(dtype, M, monkeypatch):
    """A real projection shape (GPT-J's 4096 x 4096) through the GEMV and the MFMA kernel."""
    _run_case(dtype, M, 4096, 4096, monkeypatch, seed=M)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_w8_linear_unsupported_inputs_take_the_reference_path(dtype, monkeypatch):
    """K % 16 != 0, a pointer off the 16-byte grid and a non-unit column stride: the result is the
    reference path's, bit for bit, and nothing is written around ``out``."""
    g = torch.Generator(device=dev).manual_seed(7)
    M, N = 5, 48
    calls = _spy(monkeypatch)

    def run(x, q, what):
        b = (torch.randn(N, generator=g, device=dev) * 0.1).to(dtype)
        buf = torch.full((M + 2, N + 16), 777.0, device=dev, dtype=dtype)
        ref_buf = buf.clone()
        del calls[:]
        y = w8.w8_linear(x, q, b, 1, out=buf[1:M + 1, 8:8 + N])
        assert not any(rc == 0 for _, rc in calls), (what, calls)  # no native launch
        assert torch.equal(y, w8.w8_linear_reference(x, q, b, 1)), what
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:M + 1, 8:8 + N] = False
        assert torch.equal(buf[keep], ref_buf[keep]), what

    K = 520  # 520 % 16 == 8
    q = w8.quantize_weight(torch.randn(N, K, generator=g, device=dev) * K ** -0.5)
    run((torch.randn(M, K, generator=g, device=dev) * 0.5).to(dtype), q, "K % 16")
    K = 512
    q = w8.quantize_weight(torch.randn(N, K, generator=g, device=dev) * K ** -0.5)
    flat = (torch.randn(M * K + 8, generator=g, device=dev) * 0.5).to(dtype)
    x = flat[4:4 + M * K].view(M, K)
    assert x.data_ptr() % 16 == 8
    run(x, q, "misaligned x")
    wide = (torch.randn(M, 2 * K, generator=g, device=dev) * 0.5).to(dtype)
    run(wide[:, ::2], q, "column stride 2")
    # the aligned, unit-stride twin of the last input does take the kernel
    del calls[:]
    w8.w8_linear(wide[:, ::2].contiguous(), q)
    assert calls == [("kca_w8_gemm", 0)]


# ------------------------------------------------------------------------------------------ engine
def small_lm(preset, dtype=torch.bfloat16, device=dev):
    """The shrunk presets of tests/test_decode_gpu.py (``_small_lm`` and the 1024-wide GPT-J of
    ``test_engine_batched_mfma_layer``), their four projections per block snapped onto the FP8 grid in
    place: quantization is lossless, so prefill (16-bit weights) and decode (FP8) see the same numbers.

    The final LayerNorm's gain is doubled, which doubles every logit bit for bit (a power of two). The
    top-2 gap of V random-init logits of spread s is about exponential with mean s / sqrt(2 ln V):
    0.14 for these models, so only half of the generated tokens would clear the 0.1 margin, and "at
    least half were checked" would be a coin toss; doubled, about two thirds clear it (0.53 .. 0.89 over
    72 (preset, batch, seed) runs of the CPU reference path). Two 16-bit evaluations of the same
    logits differ by one unit in the last place of a logit, 0.03 at this scale, still well inside 0.1."""
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    small = {"gpt-neox-20b": dict(hidden_size=768, num_hidden_layers=3, num_attention_heads=8,
                                  intermediate_size=3072, max_position_embeddings=512),
             "bloom-560m": dict(hidden_size=512, n_layer=3, n_head=4),
             "gpt2": dict(n_embd=512, n_layer=3, n_head=8, n_positions=512),
             "gpt-j-6b": dict(n_embd=1024, n_layer=3, n_head=4, rotary_dim=64, n_positions=512)}[preset]
    cfg = dict(PRESETS_HF[preset])
    cfg.update(small)
    m = build_model(LMConfig.from_hf(cfg), device=device, dtype=dtype, seed=0)
    with torch.no_grad():
        for blk in m.h:
            for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out):
                mod.weight.copy_(w8.snap_to_grid(mod.weight))
        m.ln_f.weight.mul_(2.0)
        if m.ln_f.bias is not None:
            m.ln_f.bias.mul_(2.0)
    return m


def make_prompts(B, seed):
    g = torch.Generator().manual_seed(seed)
    return [[int(x) for x in torch.randint(0, 1000, (int(n),), generator=g)]
            for n in torch.randint(8, 90, (B,), generator=g)]


def check_against_forward(m, prompt, out, margin=0.1):
    """tests/test_decode_gpu.py ``_check_against_forward``: every generated token whose top-2 logit margin
    in the model's full forward exceeds ``margin`` is that forward's argmax. Returns the number checked."""
    with torch.no_grad():
        lg = m(torch.tensor([prompt + out], device=next(m.parameters()).device))[0].float()
    n = 0
    for i, t in enumerate(out):
        row = lg[len(prompt) - 1 + i]
        top2 = row.topk(2).values
        if float(top2[0] - top2[1]) > margin:
            assert int(row.argmax()) == t, i
            n += 1
    return n


NEW = 16
ROUNDS = {1: 4, 3: 2, 20: 1}  # generate() calls per batch size: at least 48 tokens behind the "half" count


def _greedy_rounds(eng, m, B):
    from kubernetes_cloud_amd.engine.llm_engine import SamplingParams
    checked = total = 0
    for r in range(ROUNDS[B]):
        prompts = make_prompts(B, 10 * B + r)
        outs = [q.output for q in eng.generate(prompts, SamplingParams(max_new_tokens=NEW, do_sample=False))]
        assert all(len(o) == NEW for o in outs)
        checked += sum(check_against_forward(m, p, o) for p, o in zip(prompts, outs))
        total += NEW * B
    return checked, total


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [1, 3, 20])
def test_engine_fp8_decode(preset, B):
    """FP8 weight-only decode with HIP graphs at batch 1 (where the 16-bit engine runs the fused
    layer), 3 and 20: greedy tokens match the model's own full forward wherever its top-2 margin is
    clear, at least half of the tokens are clear, the step ran on the FP8 path alone, and a seeded
    sampled run replays bit-identically."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = small_lm(preset)
    eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, weight_dtype="fp8")
    r = eng.runner
    assert r.use_graphs and r._w8 is not None
    checked, total = _greedy_rounds(eng, m, B)
    assert r.w8_steps > 0 and r.batched_steps == 0 and r.fused_steps == 0
    print(f"{preset} B={B}: {checked} of {total} tokens checked")
    assert 2 * checked >= total
    prompts = make_prompts(B, 10 * B)
    sp = SamplingParams(max_new_tokens=10, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
    a = [q.output for q in eng.generate(prompts, sp)]
    b = [q.output for q in eng.generate(prompts, sp)]
    assert a == b and all(len(x) == 10 for x in a)


def test_engine_fp8_decode_fp16_model():
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m = small_lm("gpt-j-6b", dtype=torch.float16)
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype="fp8")
    checked, total = _greedy_rounds(eng, m, 3)
    assert eng.runner.w8_steps > 0 and eng.runner.batched_steps == 0 and eng.runner.fused_steps == 0
    assert 2 * checked >= total
