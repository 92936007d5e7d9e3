"""MXFP4 weight-only decode on the GPU: ``kca_mx4_gemm`` (csrc/kernels/gemv_mx4.hip) per element
against fp64, and ``LLMEngine(weight_dtype="mxfp4")`` against the model's own forward.

Kernel bound, per element, against ``ref = act(sum_k x[m,k] v[n,k] s[n,k/32] + bias[n])`` computed in
fp64 from the kernel's own 16-bit x, e2m1 nibbles v and e8m0 scale bytes (s = 2^(E - 127)) -- the bound
of tests/test_w8_gpu.py, derived there:

    no activation:  |y - ref| <= u * |ref| + 2^-20 * sum_k |x v s|
    activation:     |y - ref| <= u * |ref| + 1.13 * 2^-20 * sum_k |x v s| + A

u = 2^-8 (bf16) / 2^-11 (fp16): half a unit in the last place of the one output rounding. The second
term is a generous fp32 accumulation error on the sum of magnitudes; 1.13 bounds |GELU'|. A is the
allowance the existing per-element GELU tests give the activation's own evaluation: four times the
largest error of the same GELU evaluated in fp32 torch on the same pre-activations, taken from the
reference at run time. Inputs are scaled so that no output lands in fp16's subnormal range.

Engine: tokens are compared with the model's own forward wherever its top-2 margin exceeds 0.1, and
at least ONE THIRD of the generated tokens must clear it (the FP8 tests ask for half): MXFP4-snapped
weights carry about 11 % rounding noise, and fp32 CPU forwards of the four presets with snapped
weights and the doubled final gain cleared the margin for 0.44 .. 1.00 of their own greedy tokens
(16 runs of 16 to 48 tokens; the lowest, 0.44, a 16-token run of the NeoX preset).
"""
import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd.ops import _lib, mx4

from .test_w8_gpu import NEW, ROUNDS, check_against_forward, make_prompts

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130]
NKS = [(16, 32), (272, 512), (1360, 992), (640, 6208)]
BIG, TINY = 127 + 14, 127 - 30  # the scale bytes of the planted fp16-range row


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
    """Quantized random rows with planted ones: row 0 all nibbles 0, row 1 alternating +6 / -6 under a
    small scale (2^-8), row 2 salted with 0x8 (-0) nibbles in both halves of a byte, row 3 with blocks
    alternating the scale bytes 127 + 14 and 127 - 30 (6 * 2^14 overflows fp16, 0.5 * 2^-30 is below
    its subnormals: only a block scale applied in fp32 survives). A weight of one block (K = 32) cannot
    alternate and has no row 3: with its only block large, all of x would be scaled down (``_x``) and
    every row's outputs would sink into fp16's subnormals, which the bound excludes."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = mx4.quantize_weight(torch.randn(N, K, generator=g, device=dev) * K ** -0.5)
    q.q[0] = 0
    q.q[1] = 0xF7
    q.scale[1] = 127 - 8
    q.q[2, ::5] = (q.q[2, ::5] & 0xF0) | 0x08
    q.q[2, 1::7] = (q.q[2, 1::7] & 0x0F) | 0x80
    if K >= 64:
        blk = torch.arange(K // 32, device=dev)
        q.scale[3] = torch.where(blk % 2 == 0, BIG, TINY).to(torch.uint8)
    assert not (q.scale == 0xFF).any()
    return q, g


def _x(M, K, g, dtype):
    """x inside a wider buffer (ldx > K); half-scale rows keep GELU outputs out of fp16's subnormals;
    the columns of row 3's large blocks (``_weights``; K >= 64) are scaled by 2^-10 so that its outputs
    stay finite."""
    xf = torch.randn(M, K + 24, generator=g, device=dev) * 0.5
    if K >= 64:
        k = torch.arange(K + 24, device=dev)
        xf[:, (k // 32) % 2 == 0] *= 2.0 ** -10
    return xf.to(dtype)[:, :K]


def _act(z, act):
    return F.gelu(z, approximate="tanh") if act == 1 else F.gelu(z) if act == 2 else z


def _ref(x, q, bias, act):
    """(ref, bound) of the module docstring, in fp64."""
    N = q.q.shape[0]
    wd = (q.values(torch.float64).view(N, -1, 32) * q.scales(torch.float64)[:, :, None]).view(N, -1)
    xd = x.double()
    z = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if bias is not None:
        z = z + bias.double()
    ref = _act(z, act)
    tol = U[x.dtype] * ref.abs() + (1.13 if act else 1.0) * 2.0 ** -20 * mag
    if act:
        tol = tol + 4 * (_act(z.float(), act).double() - ref).abs().max()
    return ref, tol


def _check(y, ref, tol, what):
    """Prints the worst error / bound ratio before asserting."""
    err = (y.double() - ref).abs()
    ok = err <= tol  # (a NaN or inf output compares False)
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}")
    assert bool(ok.all()), (what, int((~ok).sum()), err[~ok].max().item(), ratio)


def _run_case(dtype, M, N, K, monkeypatch, seed):
    q, g = _weights(N, K, seed)
    x = _x(M, K, g, dtype)
    assert x.stride(0) == K + 24
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(dtype)
    calls = _spy(monkeypatch)
    launches = -(-M // mx4.MAX_M)
    for act in (0, 1, 2):
        for bias in (None, b):
            ref, tol = _ref(x, q, bias, act)  # one reference per (act, bias), shared by both strides
            assert bool(torch.isfinite(ref).all())
            for pad in (24, 13):  # row stride N + 24: 8-byte-aligned rows (packed stores); N + 13: scalar stores
                buf = torch.full((M + 2, 8 + N + pad - 8), 777.0, device=dev, dtype=dtype)
                ref_buf = buf.clone()
                out = buf[1:M + 1, 8:8 + N]
                del calls[:]
                y = mx4.mx4_linear(x, q, bias, act, out=out)
                assert y.data_ptr() == out.data_ptr()
                assert calls == [("kca_mx4_gemm", 0)] * launches, calls  # the native kernel, one launch per slab
                what = f"mx4 {dtype} M={M} N={N} K={K} act={act} bias={bias is not None} ldy=N+{pad}"
                _check(y, ref, tol, what)
                # guard rows and columns of the sentinel buffer untouched
                keep = torch.ones_like(buf, dtype=torch.bool)
                keep[1:M + 1, 8:8 + N] = False
                assert torch.equal(buf[keep], ref_buf[keep]), what
                # planted row 0: all nibbles 0 gives exactly 0, or the bias where nothing else rounds
                if bias is None or act == 0:
                    z0 = torch.zeros(M, device=dev, dtype=dtype) if bias is None else bias[0].expand(M)
                    assert torch.equal(y[:, 0], z0), what
                # the same call gives the same bits, with and without `out`
                y2 = mx4.mx4_linear(x, q, bias, act)
                assert torch.equal(y2, y), what


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_gemm_per_element(dtype, N, K, M, monkeypatch):
    """Every boundary of the kernels: M = 1..4 (GEMV, row pads 1 / 2 / 4), 5..64 (MFMA, 1 / 2 / 4
    activation tiles), 65 and 130 (the 64-row slab loop); the smallest legal shape (one block, one
    workgroup); an odd number of 16-row workgroups (272 = 17 * 16, 1360 = 85 * 16); K off the 128-wide
    chunk (992 = 7 * 128 + 96: a chunk of three blocks) and off the GEMV's 4096-wide step and the MFMA
    kernel's 1024-wide round of chunks (6208 = 194 blocks); every activation, with and without bias,
    both store forms."""
    _run_case(dtype, M, N, K, monkeypatch, seed=M * 131 + N + K)


@pytest.mark.parametrize("M", [3, 7])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_gemm_rows_past_n(dtype, M, monkeypatch):
    """N = 37: the shapes above are all multiples of the 16 rows of a workgroup, so this is the case
    where waves and lanes own rows past N (read from a valid row, never stored) and where a lane's four
    output rows straddle N (the packed store's scalar tail)."""
    _run_case(dtype, M, 37, 96, monkeypatch, seed=M)


@pytest.mark.parametrize("N,M", [(8232, 8), (8232, 32), (16376, 8), (16376, 32), (16376, 40)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_gemm_wide_n(dtype, N, M, monkeypatch):
    """From 512 16-row tiles on, a workgroup of the MFMA kernel owns two of them (M <= 32), and four
    where that makes whole rounds of 256 workgroups (M <= 16). N = 8232 is 514.5 tiles: pairs, the last
    workgroup with a partial tile and a tile wholly past N. N = 16376 is 1023.5 tiles: 256 workgroups of
    four at M = 8 (the last with a partial tile), pairs at M = 32, single tiles at M = 40. K = 96 keeps
    it small (three blocks: seven of the eight waves have nothing but the fan-in to do)."""
    _run_case(dtype, M, N, 96, monkeypatch, seed=N + M)


@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_gemm_projection_shape(dtype, M, monkeypatch):
    """A real projection shape (GPT-J's 4096 x 4096) through the GEMV and the MFMA kernel."""
    _run_case(dtype, M, 4096, 4096, monkeypatch, seed=M)


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_gemm_exact_integers(dtype, M, monkeypatch):
    """Settles the nibble / byte order of the conversion against the packing: small integers in x (20
    nonzeros of +-1, +-2 per row at scattered odd and even k), weights among +-{1, 2, 3, 4, 6} with all
    scale bytes 127, no two rows or columns alike. |y| <= 20 * 2 * 6 = 240: every partial sum is an
    integer below 2^8, exact in fp32 and in both 16-bit types, so the result equals the reference bit for
    bit whatever the summation order."""
    N, K = 48, 128
    g = torch.Generator().manual_seed(11 + M)
    codes = torch.tensor([2, 4, 5, 6, 7], dtype=torch.uint8)  # 1, 2, 3, 4, 6
    nib = codes[torch.randint(0, 5, (N, K), generator=g)] | (torch.randint(0, 2, (N, K), generator=g).to(torch.uint8) << 3)
    q = mx4.MX4Weight((nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous().to(dev),
                      torch.full((N, K // 32), 127, dtype=torch.uint8, device=dev))
    x = torch.zeros(M, K)
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    for m in range(M):
        x[m, torch.randperm(K, generator=g)[:20]] = vals[torch.randint(0, 4, (20,), generator=g)]
    assert len({tuple(r.tolist()) for r in nib}) == N and len({tuple(c.tolist()) for c in nib.t()}) == K
    assert len({tuple(r.tolist()) for r in x}) == M
    x = x.to(dev, dtype)
    ref = x.double() @ q.values(torch.float64).t()
    assert float(ref.abs().max()) <= 240 and torch.equal(ref.to(dtype).double(), ref)
    calls = _spy(monkeypatch)
    y = mx4.mx4_linear(x, q)
    assert calls == [("kca_mx4_gemm", 0)]
    bad = (y.double() != ref).nonzero()
    assert torch.equal(y.double(), ref), (bad[:8].tolist(), y[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    assert torch.equal(y, mx4.mx4_linear_reference(x, q))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx4_linear_unsupported_inputs_take_the_reference_path(dtype, monkeypatch):
    """A pointer off the 16-byte grid, a non-unit column stride and fp32 x: the result is the reference
    path's, bit for bit, and nothing is written around ``out``."""
    g = torch.Generator(device=dev).manual_seed(7)
    M, N, K = 5, 48, 512
    calls = _spy(monkeypatch)
    q = mx4.quantize_weight(torch.randn(N, K, generator=g, device=dev) * K ** -0.5)

    def run(x, what):
        b = (torch.randn(N, generator=g, device=dev) * 0.1).to(x.dtype)
        buf = torch.full((M + 2, N + 16), 777.0, device=dev, dtype=x.dtype)
        ref_buf = buf.clone()
        del calls[:]
        y = mx4.mx4_linear(x, q, b, 1, out=buf[1:M + 1, 8:8 + N])
        assert not any(rc == 0 for _, rc in calls), (what, calls)  # no native launch
        assert torch.equal(y, mx4.mx4_linear_reference(x, q, b, 1)), what
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:M + 1, 8:8 + N] = False
        assert torch.equal(buf[keep], ref_buf[keep]), what

    flat = (torch.randn(M * K + 8, generator=g, device=dev) * 0.5).to(dtype)
    x = flat[4:4 + M * K].view(M, K)
    assert x.data_ptr() % 16 == 8
    run(x, "misaligned x")
    wide = (torch.randn(M, 2 * K, generator=g, device=dev) * 0.5).to(dtype)
    run(wide[:, ::2], "column stride 2")
    run(torch.randn(M, K, generator=g, device=dev) * 0.5, "fp32 x")
    # the aligned, unit-stride twin does take the kernel
    del calls[:]
    mx4.mx4_linear(wide[:, ::2].contiguous(), q)
    assert calls == [("kca_mx4_gemm", 0)]


# ------------------------------------------------------------------------------------------ engine
def small_lm(preset, dtype=torch.bfloat16, device=dev):
    """tests/test_w8_gpu.py ``small_lm`` with the four projections per block snapped onto the MXFP4
    grid instead: quantization is lossless, so prefill (16-bit weights) and decode (MXFP4) see the same
    numbers. The final LayerNorm's gain is doubled as there (every logit doubles bit for bit)."""
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
                mod.weight.copy_(mx4.snap_to_grid(mod.weight))
        m.ln_f.weight.mul_(2.0)
        if m.ln_f.bias is not None:
            m.ln_f.bias.mul_(2.0)
    return m


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


def _only_mx4_steps(r):
    return r.mx4_steps > 0 and r.w8_steps == 0 and r.batched_steps == 0 and r.fused_steps == 0


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [1, 3, 20])
def test_engine_mxfp4_decode(preset, B):
    """MXFP4 weight-only decode with HIP graphs at batch 1 (where the 16-bit engine runs the fused
    layer), 3 and 20: greedy tokens match the model's own full forward wherever its top-2 margin is
    clear, at least a third of the tokens are clear (module docstring), the step ran on the MXFP4 path
    alone, the quantized weights reproduce the snapped ones, and a seeded sampled run replays
    bit-identically."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = small_lm(preset)
    eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, weight_dtype="mxfp4")
    r = eng.runner
    assert r.use_graphs and r._mx4 is not None and r._w8 is None and len(r._mx4) == 4 * len(m.h)
    w = m.h[0].mlp.fc_out
    assert torch.equal(mx4.dequantize(r._mx4[id(w)], w.weight.dtype), w.weight)
    checked, total = _greedy_rounds(eng, m, B)
    assert _only_mx4_steps(r)
    print(f"{preset} B={B}: {checked} of {total} tokens checked")
    assert 3 * checked >= total
    prompts = make_prompts(B, 10 * B)
    sp = SamplingParams(max_new_tokens=10, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
    a = [q.output for q in eng.generate(prompts, sp)]
    b = [q.output for q in eng.generate(prompts, sp)]
    assert a == b and all(len(x) == 10 for x in a)


def test_engine_mxfp4_decode_fp16_model():
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine
    m = small_lm("gpt-j-6b", dtype=torch.float16)
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype="mxfp4")
    checked, total = _greedy_rounds(eng, m, 3)
    assert _only_mx4_steps(eng.runner)
    print(f"fp16: {checked} of {total} tokens checked")
    assert 3 * checked >= total


def test_engine_mxfp4_with_fp8_kv():
    """Both options: the reference is the FP8-KV tests' (tests/test_kv8_gpu.py) -- a CPU fp32 copy of
    the model behind an FP8 KV cache, teacher-forced with the tokens under test -- at their margin for
    this preset and batch, since the cache's quantization moves the logits away from the plain forward."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine

    from .test_kv8_gpu import _cpu_copy, _margin
    from .test_kv8_gpu import _greedy_rounds as kv8_rounds
    m = small_lm("gpt-j-6b")
    eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True, weight_dtype="mxfp4", kv_dtype="fp8")
    checked, total = kv8_rounds(eng, _cpu_copy(m, "gpt-j-6b"), 3, 256, _margin(("gpt-j-6b", 3)))
    r = eng.runner
    assert _only_mx4_steps(r) and r.kv8_steps == r.mx4_steps
    print(f"mxfp4 + kv8: {checked} of {total} tokens checked")
    assert 3 * checked >= total
