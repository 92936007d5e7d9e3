"""Prefix caching on the GPU: ``kca_prefill_paged_attn`` (csrc/kernels/prefill_paged.hip) per element against
the float64 oracle of tests/attention_ref.py on the gathered keys, its exact properties (zeros for padding,
nothing written around ``out``, paged == contiguous, a row alone == the row in a batch, run to run,
causality at the tile edges), and the engine with ``prefix_cache=True`` on the shrunk presets.

Bounds are the project's: bf16 outputs are held to ``attention_ref.fwd``'s ``bound_o`` through
``assert_within``; fp16 outputs to ``_within`` of tests/test_decode_fp16_gpu.py (two units in the last place
plus four times the error of the fp32 reference on the same inputs)."""
import math

import pytest
import torch

from kubernetes_cloud_amd.ops import prefill_paged as pp

from . import attention_ref as ar
from .test_decode_fp16_gpu import _within
from .test_decode_gpu import _paginate

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

ROW_SLOTS = (3, 0, 2, 1)  # of 5 slots: slot 4 is never used
SLOTS, T, LMAX, HKV = 5, 130, 320, 2
# (start, len): one query on an empty slot; a fresh prompt; a chunk that starts on a page boundary of PS = 16
# and ends mid-tile; a mid-page start with two query tiles (128 + 2) and keys across 17 / 5 pages
ROWS = ((0, 1), (0, 70), (48, 33), (131, 130))
NAN = float("nan")


def _case(D, G, PS, dtype, alibi, seed=0):
    """Inputs of one launch. Every cache position a query may not read -- the unused slot, the scratch
    page, the positions at or past start + len -- and every padding query is NaN: one over-read poisons
    the output."""
    g = torch.Generator().manual_seed(1000 * D + 10 * G + seed)
    H = HKV * G
    k = torch.randn(SLOTS, HKV, LMAX, D, generator=g)
    v = torch.randn(SLOTS, HKV, LMAX, D, generator=g)
    qkv = torch.randn(len(ROWS), T, 3, H, D, generator=g)
    k[4], v[4] = NAN, NAN
    for s_, (p0, n) in zip(ROW_SLOTS, ROWS):
        k[s_, :, p0 + n:], v[s_, :, p0 + n:] = NAN, NAN
    for r, (p0, n) in enumerate(ROWS):
        qkv[r, n:] = NAN
    k, v, qkv = k.to(dtype).to(dev), v.to(dtype).to(dev), qkv.to(dtype).to(dev)
    slopes = (2.0 ** -(torch.arange(H, dtype=torch.float32) + 1) * 0.5).to(dev) if alibi else None
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731
    return dict(q=qkv[:, :, 0], k=k, v=v, H=H, D=D, scale=1.0 / math.sqrt(D), alibi=slopes, slots=i32(ROW_SLOTS),
                start=i32([p0 for p0, _ in ROWS]), lens=i32([n for _, n in ROWS]), dtype=dtype)


def _caches(c, PS):
    """(k cache, v cache, block table) of the case: contiguous (PS = 0) or shuffled pages, scratch page NaN."""
    if not PS:
        return c["k"], c["v"], None
    kp, tbl = _paginate(c["k"], PS, 5)
    vp, _ = _paginate(c["v"], PS, 5)
    kp[-1], vp[-1] = NAN, NAN
    return kp, vp, tbl


def _launch(c, PS, rows=None):
    """The op on the case (or on ``rows`` of it) into a 777-filled buffer with a guard band around ``out``:
    returns (out, buffer, untouched-mask)."""
    kc, vc, tbl = _caches(c, PS)
    rows = list(range(len(ROWS))) if rows is None else rows
    n, H, D = len(rows), c["H"], c["D"]
    buf = torch.full((n + 2, T + 1, H, D + 8), 777.0, device=dev, dtype=c["dtype"])
    out = buf[1:n + 1, :T, :, :D]
    idx = torch.tensor(rows, device=dev)
    y = pp.prefill_paged_attention(c["q"][idx] if rows != list(range(len(ROWS))) else c["q"], kc, vc,
                                   c["slots"][idx].contiguous(), c["start"][idx].contiguous(),
                                   c["lens"][idx].contiguous(), c["scale"], c["alibi"], out=out, block_table=tbl)
    assert y.data_ptr() == out.data_ptr()
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:n + 1, :T, :, :D] = False
    return out, buf, keep


def _oracle(c, r):
    """attention_ref.fwd (float64) of row r on its gathered keys: (o, bound_o), [len, H, D]."""
    p0, n = ROWS[r]
    s_ = ROW_SLOTS[r]
    kg = c["k"][s_, :, :p0 + n].transpose(0, 1)[None]
    vg = c["v"][s_, :, :p0 + n].transpose(0, 1)[None]
    f = ar.fwd(c["q"][r:r + 1, :n], kg, vg, True, c["scale"], alibi=c["alibi"])
    return f["o"][0], f["bound_o"][0]


CASES = [(64, 1, 0, torch.bfloat16, False), (64, 1, 16, torch.float16, True), (96, 1, 16, torch.bfloat16, True),
         (96, 1, 64, torch.float16, False), (128, 4, 64, torch.bfloat16, True), (128, 4, 0, torch.float16, False),
         (256, 1, 0, torch.bfloat16, True), (256, 1, 64, torch.float16, False), (256, 1, 16, torch.bfloat16, False)]


@pytest.mark.parametrize("D,G,PS,dtype,alibi", CASES)
def test_kernel_per_element(D, G, PS, dtype, alibi):
    """One launch of four rows in slots (3, 0, 2, 1): every real query within the bound of its format, padding
    queries exactly zero, the guard band untouched."""
    assert pp.supported(D, HKV * G, HKV, 0)
    c = _case(D, G, PS, dtype, alibi)
    out, buf, keep = _launch(c, PS)
    torch.cuda.synchronize()
    assert bool((buf[keep] == 777.0).all())
    y32 = None
    if dtype == torch.float16:
        kc, vc, tbl = _caches(c, PS)
        y32 = pp.prefill_paged_attention_reference(c["q"].float(), kc.float(), vc.float(), c["slots"], c["start"],
                                                   c["lens"], c["scale"], c["alibi"], block_table=tbl)
    for r, (p0, n) in enumerate(ROWS):
        what = f"prefill_paged D={D} G={G} PS={PS} {dtype} alibi={alibi} row {r} (start {p0}, len {n})"
        assert not out[r, n:].any(), what  # padding queries: zeros, bit for bit
        o64, bound = _oracle(c, r)
        if dtype == torch.bfloat16:
            ar.assert_within(what, out[r, :n], o64, bound)
        else:
            _within(out[r, :n], o64.to(dev), y32[r, :n], what)


@pytest.mark.parametrize("D,G,dtype,alibi", [(64, 1, torch.bfloat16, True), (128, 4, torch.float16, False),
                                             (256, 1, torch.bfloat16, False)])
def test_kernel_exact_properties(D, G, dtype, alibi):
    c = _case(D, G, 16, dtype, alibi, seed=1)
    out, buf, keep = _launch(c, 16)
    # two runs, bit for bit
    again, _, _ = _launch(c, 16)
    assert torch.equal(out, again)
    # paged (PS = 16, shuffled pages) == contiguous
    flat, fbuf, fkeep = _launch(c, 0)
    assert torch.equal(out, flat)
    assert bool((buf[keep] == 777.0).all()) and bool((fbuf[fkeep] == 777.0).all())
    # padding queries and a padded row (len 1 of T = 130: the second query tile is all padding) are zeros
    for r, (p0, n) in enumerate(ROWS):
        assert not out[r, n:].any() and bool(torch.isfinite(out[r, :n].float()).all())
    # a row launched alone == the same row inside the batch
    for r in range(len(ROWS)):
        alone, abuf, akeep = _launch(c, 16, rows=[r])
        assert torch.equal(alone[0], out[r]), r
        assert bool((abuf[akeep] == 777.0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("jstar", [31, 32, 97])
def test_kernel_causality(jstar, dtype):
    """K and V at position start + j* of the last row scaled by 2^10 (a tile's last key, the next tile's
    first, an interior key): queries before j* keep their bits, every query from j* on changes."""
    c = _case(128, 1, 16, dtype, False, seed=2)
    base, _, _ = _launch(c, 16)
    r = len(ROWS) - 1
    p0, n = ROWS[r]
    c["k"][ROW_SLOTS[r], :, p0 + jstar] *= 1024.0
    c["v"][ROW_SLOTS[r], :, p0 + jstar] *= 1024.0
    moved, _, _ = _launch(c, 16)
    assert torch.equal(moved[:r], base[:r])  # the other rows read other slots
    assert torch.equal(moved[r, :jstar], base[r, :jstar])
    changed = (moved[r, jstar:n] != base[r, jstar:n]).flatten(1).any(1)
    assert bool(changed.all()), (~changed).nonzero().flatten().tolist()
    assert torch.equal(moved[r, n:], base[r, n:])


def test_unsupported_arguments_raise():
    c = _case(64, 1, 0, torch.bfloat16, False)
    with pytest.raises(RuntimeError, match="kca_prefill_paged_attn"):  # a token stride off the 16-byte grid
        pp.prefill_paged_attention(c["q"].reshape(len(ROWS), T, -1)[:, :, 4:4 + 64].unflatten(2, (1, 64)),
                                   c["k"], c["v"], c["slots"], c["start"], c["lens"], c["scale"])
    assert not pp.supported(64, 4, 4, 256) and not pp.supported(260, 4, 4, 0) and not pp.supported(64, 6, 4, 0)
    assert not pp.supported(68, 4, 4, 0) and pp.supported(72, 4, 4, 0) and pp.supported(256, 16, 16)


# ------------------------------------------------------------------------------------------ engine
PREFIX_SEED, NEW = 3, 16


def engine_prompts(seed=PREFIX_SEED):
    """(the first request, the batch that follows): all share a 64-token prefix -- one page of the default
    page size -- and end in tails of 5..40 tokens of their own."""
    g = torch.Generator().manual_seed(seed)
    prefix = [int(x) for x in torch.randint(0, 1000, (64,), generator=g)]
    tails = [[int(x) for x in torch.randint(0, 1000, (n,), generator=g)] for n in (12, 5, 40, 23, 9, 31)]
    return prefix + tails[0], [prefix + t for t in tails[1:]]


def run_engine(m, ref, **kw):
    """The scenario on model ``m`` (checked against ``ref``'s full forward): returns (engine, checked, total)."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from .test_w8_gpu import check_against_forward
    on_gpu = next(m.parameters()).is_cuda
    eng = LLMEngine(m, max_slots=8, max_len=256, use_graphs=on_gpu, prefix_cache=True, **kw)
    first, batch = engine_prompts()
    sp = SamplingParams(max_new_tokens=NEW, do_sample=False)
    checked = total = 0
    for prompts in ([first], batch):
        outs = [r.output for r in eng.generate(prompts, sp)]
        assert all(len(o) == NEW for o in outs)
        checked += sum(check_against_forward(ref, p, o) for p, o in zip(prompts, outs))
        total += NEW * len(prompts)
    return eng, checked, total


def _engine_asserts(eng, checked, total, what):
    r = eng.runner
    print(f"{what}: {checked} of {total} tokens checked, {eng.stats['prefix_hit_tokens']} prefix tokens hit, "
          f"{r.paged_prefill_calls} paged / {r.gather_prefill_calls} gather layer calls")
    assert r.paged_prefill_calls > 0 and r.gather_prefill_calls == 0
    assert eng.stats["prefix_hit_tokens"] == 5 * 64 and eng.stats["prefix_lookups"] == 6
    assert 2 * checked >= total


@pytest.mark.parametrize("preset,dtype", [("gpt-j-6b", torch.bfloat16), ("gpt-neox-20b", torch.bfloat16),
                                          ("bloom-560m", torch.bfloat16), ("gpt2", torch.bfloat16),
                                          ("gpt-j-6b", torch.float16), ("bloom-560m", torch.float16)])
def test_engine_prefix_hits(preset, dtype):
    """A first request fills the shared 64-token page; the batch of five that follows adopts it and
    prefills only its tails, through the paged kernel alone, with HIP graphs on. Every generated token
    whose top-2 margin in the model's own full forward is clear is that forward's argmax, and at least
    half of the tokens are clear (the condition of ``test_engine_fp8_decode``). The prompts
    (``engine_prompts``) were checked with the CPU reference path (``run_engine`` on CPU models of the
    same dtype): there the scenario clears 65 to 96 of the 96 tokens on every (preset, dtype) used here
    (GPT-J 68 / 69 in bf16 / fp16, NeoX 65, GPT-2 65, BLOOM 96 / 96; 72 in the MXFP4 run below), so the
    half does not hang on the kernel."""
    from .test_w8_gpu import small_lm
    m = small_lm(preset, dtype)
    eng, checked, total = run_engine(m, m)
    assert eng.runner.use_graphs
    _engine_asserts(eng, checked, total, f"{preset} {dtype}")


def test_engine_prefix_hits_quantized_prefill():
    """The same with MXFP4 weights in prefill and decode on the MXFP4-snapped model (quantization is
    lossless there; its 16-bit projection weights are released, so a twin gives the full forward)."""
    from .test_mx4_gpu import small_lm
    m, ref = small_lm("gpt-j-6b"), small_lm("gpt-j-6b")
    eng, checked, total = run_engine(m, ref, weight_dtype="mxfp4", prefill_weights="quantized")
    assert eng.runner.wq_prefill_steps > 0 and eng.runner.mx4_steps > 0
    _engine_asserts(eng, checked, total, "gpt-j-6b mxfp4 quantized prefill")
