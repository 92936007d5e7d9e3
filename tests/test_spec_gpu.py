"""Speculative decoding on the GPU (csrc/kernels/decode_spec.hip through ops/spec.py and the engine).

Prep: bf16 bytes against ``kca_decode_prep`` on the same rows, bit for bit; fp16 against an fp64 rotation
under the bound tests/test_kv8_gpu.py ``test_kv8_prep`` uses for its fp16 rotation. Attention: per element
against ``spec_attention_reference(fp64=True)`` under tests/test_decode_fp16_gpu.py's bound (``_within``:
two units in the last place of the output plus four times the error of the fp32 reference), with edges
planted so that a key leaking into an earlier query's softmax cannot hide inside the bound. Engine: a
scripted proposer with every fifth draft wrong, behind HIP graphs, against the model's own full forward.
"""
import pytest
import torch

from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops import spec
from kubernetes_cloud_amd.ops.rope import rope_tables

from .test_decode_fp16_gpu import _within
from .test_decode_gpu import _paginate
from .test_kv8_gpu import _rotate64
from .test_spec_cpu import Scripted, implied
from .test_w8_gpu import NEW, ROUNDS, check_against_forward, make_prompts, small_lm

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
BF16, F16 = torch.bfloat16, torch.float16
NAN = float("nan")


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _i32(xs):
    return torch.tensor(list(xs), device=dev, dtype=torch.int32)


# ------------------------------------------------------------------------------------------ prep
@pytest.mark.parametrize("H,Hkv,D,rot,inter", [(4, 4, 64, 0, False), (4, 4, 256, 64, True), (8, 8, 96, 24, False),
                                               (8, 2, 128, 128, False)])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("PS", [0, 16])
def test_spec_prep(H, Hkv, D, rot, inter, dtype, PS):
    """kca_spec_prep on 3 sequences x T = 4 rows, n_tok = (4, 3, 1), the second sequence's tokens across a
    page boundary (positions 14..16). bf16: the rotated Q and the whole NaN-filled caches are bit-equal to
    what kca_decode_prep leaves when given the real rows. fp16 (no kca_decode_prep twin): V rows and the
    unrotated dims bit-equal to the input, rotated Q and K held to the fp64 rotation under test_kv8_prep's
    fp16 bound -- half a unit in the last place (2^-11 |ref|), 2^-20 (|x| + |partner|) for the two fp32
    products and their sum, and half the smallest subnormal. Rows t >= n_tok leave Q and the caches alone."""
    g = _gen(D + rot + PS)
    B, T, S, L = 3, 4, 4, 32
    qkv = (torch.randn(B * T, (H + 2 * Hkv) * D, generator=g, device=dev) * 2).to(dtype)
    base, n_tok, slots = _i32([0, 14, 27]), _i32([4, 3, 1]), _i32([2, 0, 3])
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    shape = (S * (L // PS) + 1, Hkv, PS, D) if PS else (S, Hkv, L, D)
    tbl = None
    if PS:
        tbl = torch.randperm(S * (L // PS), generator=torch.Generator().manual_seed(1)).view(S, L // PS)
        tbl = tbl.to(torch.int32).to(dev)
    kc = torch.full(shape, NAN, dtype=dtype, device=dev)
    vc = torch.full(shape, NAN, dtype=dtype, device=dev)
    got = qkv.clone()
    spec.spec_prep(got, H, Hkv, D, rot, inter, cos, sin, base, n_tok, slots, T, kc, vc, tbl)
    torch.cuda.synchronize()

    rows = [(b, t) for b in range(B) for t in range(int(n_tok[b]))]
    idx = torch.tensor([b * T + t for b, t in rows], device=dev)
    pos = _i32(int(base[b]) + t for b, t in rows)
    sl = _i32(int(slots[b]) for b, _ in rows)
    pad = torch.ones(B * T, dtype=torch.bool, device=dev)
    pad[idx] = False
    assert torch.equal(got[pad], qkv[pad])  # padding rows: untouched
    # the (page or slot, row) of every written position
    wsl, wp = sl.long(), pos.long()
    if PS:
        wsl, wp = tbl.long()[wsl, wp // PS], wp % PS
    live = torch.zeros(shape[:-1], dtype=torch.bool, device=dev)
    live[wsl, :, wp] = True
    assert int(live.sum()) == len(rows) * Hkv
    for c in (kc, vc):
        assert bool(torch.isnan(c[~live]).all()) and bool(torch.isfinite(c[live]).all())
    rows_in = qkv[idx].view(len(rows), H + 2 * Hkv, D)
    assert torch.equal(got[idx].view(len(rows), -1, D)[:, H:], rows_in[:, H:])  # K / V of the row itself: as given
    assert torch.equal(vc[wsl, :, wp], rows_in[:, H + Hkv:])
    if dtype == BF16:
        sub = qkv[idx].contiguous()
        k2, v2 = torch.full_like(kc, NAN), torch.full_like(vc, NAN)
        dops.decode_prep(sub, H, Hkv, D, rot, inter, cos, sin, pos, sl, k2, v2, tbl)
        torch.cuda.synchronize()
        assert torch.equal(got[idx], sub)
        assert torch.equal(kc.view(torch.int16), k2.view(torch.int16))
        assert torch.equal(vc.view(torch.int16), v2.view(torch.int16))
        return
    for what, a, b in (("Q", 0, H), ("K", H, H + Hkv)):
        x = rows_in[:, a:b].double().abs()
        ref = _rotate64(rows_in[:, a:b], rot, inter, cos, sin, pos)
        partner = x.clone()
        if rot:
            xr = x[..., :rot]
            partner[..., :rot] = (xr.reshape(len(rows), b - a, rot // 2, 2).flip(-1).reshape(len(rows), b - a, rot)
                                  if inter else torch.cat((xr[..., rot // 2:], xr[..., :rot // 2]), -1))
        tol = 2.0 ** -11 * ref.abs() + 2.0 ** -20 * (x + partner) + 2.0 ** -25
        y = (got[idx].view(len(rows), -1, D)[:, :H] if what == "Q" else kc[wsl, :, wp]).double()
        err = (y - ref).abs()
        print(f"fp16 {what}: worst err / bound {(err / tol).max().item():.3f}")
        assert bool((err <= tol).all()), what
        assert torch.equal(y[..., rot:], rows_in[:, a:b, rot:].double())


# ------------------------------------------------------------------------------------- attention
L_MAX, S_SLOTS, HKV = 336, 4, 2
SLOTS = (2, 0, 1)


def _attn_case(D, G, T, PS, dtype, seed):
    """16-bit caches for 3 sequences in slots (2, 0, 1) of 4 (+ the paged pool's scratch page), live
    lengths (336, 130, T). Planted: the K rows of each sequence's last T - 1 positions scaled by 2^10 (a
    key that leaks to an earlier query takes over its softmax), one all-zero K / V row, and NaN everywhere
    past a sequence's length, in the unused slot and in the scratch page."""
    g = _gen(seed)
    H = HKV * G
    lens = (L_MAX, 130, T)
    kf = torch.randn(S_SLOTS, HKV, L_MAX, D, generator=g, device=dev)
    vf = torch.randn(S_SLOTS, HKV, L_MAX, D, generator=g, device=dev)
    kf[0, 0, 7] = 0.0  # sequence 2 (slot 0)
    vf[0, 0, 7] = 0.0
    vf[2, 1, 9] = 0.0
    for s_, n in zip(SLOTS, lens):
        kf[s_, :, n - (T - 1):n] *= 2.0 ** 10
        kf[s_, :, n:] = NAN
        vf[s_, :, n:] = NAN
    kf[3], vf[3] = NAN, NAN
    kc, vc, tbl = kf.to(dtype), vf.to(dtype), None
    if PS:
        kc, tbl = _paginate(kc, PS, 3)
        vc, _ = _paginate(vc, PS, 3)
        kc[-1], vc[-1] = NAN, NAN  # the scratch page
    q = torch.randn(3 * T, (H + 2 * HKV) * D, generator=g, device=dev).to(dtype)
    return q, kc, vc, tbl, H, lens


def _refs(q, kc, vc, lens, n_tok, T, H, scale, alibi, tbl, window):
    """(fp64 reference, the same reference in fp32), computed once per (lengths, n_tok)."""
    out = []
    for f64 in (True, False):
        o = torch.empty(q.shape[0], H * kc.shape[3], device=dev, dtype=torch.float64 if f64 else torch.float32)
        out.append(spec.spec_attention_reference(q, kc, vc, _i32(SLOTS), lens, n_tok, T, H, scale, alibi, o, tbl,
                                                 window, fp64=f64))
    return out


def _attn_check(q, kc, vc, lens, n_tok, T, H, scale, alibi, tbl, window, chunk, ws, refs, what):
    D = kc.shape[3]
    out = torch.full((q.shape[0], H * D), NAN, device=dev, dtype=q.dtype)
    args = (q, kc, vc, _i32(SLOTS), lens, n_tok, T, H, L_MAX, scale, alibi)
    y = spec.spec_attention(*args, out=out, ws=ws, chunk=chunk, block_table=tbl, window=window).clone()
    y2 = spec.spec_attention(*args, out=out, ws=ws, chunk=chunk, block_table=tbl, window=window)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), what
    assert torch.equal(y, y2), what  # the same call twice: the same bits
    pad = (torch.arange(T, device=dev)[None] >= n_tok[:, None]).reshape(-1)
    assert not bool(y[pad].any()), what  # rows t >= n_tok: exactly zero
    _within(y, refs[0], refs[1], what)


@pytest.mark.parametrize("D", [64, 96, 128, 256])
@pytest.mark.parametrize("G,T", [(1, 2), (1, 4), (1, 8), (2, 4), (4, 2)])
@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("window", [0, 40])
@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_spec_attention(D, G, T, alibi, window, PS, dtype):
    """kca_spec_attn per element, kv_lens = (336, 130, T): n_tok = (T, min(T, 4), T) -- the second
    sequence's tokens across the 128-token split and page boundary, the third with an empty cache before
    the step -- under the default ``decode_chunk`` split, 64-token splits (six, empty ones under the
    window) and one 512-token split; then n_tok = (1, T - 1, 1), and the same workspace with other
    lengths."""
    q, kc, vc, tbl, H, lens = _attn_case(D, G, T, PS, dtype, D + G + T + PS)
    lens = _i32(lens)
    al = (2.0 ** -torch.arange(1, H + 1, device=dev, dtype=torch.float32)) if alibi else None
    scale = D ** -0.5
    ws = torch.zeros(dops.decode_ws_floats(3 * T, H, HKV, D, L_MAX, 64) + 16, device=dev, dtype=torch.float32)
    what = f"D={D} G={G} T={T} alibi={alibi} window={window} PS={PS}"
    n_tok = _i32((T, min(T, 4), T))
    refs = _refs(q, kc, vc, lens, n_tok, T, H, scale, al, tbl, window)
    for chunk in (0, 64, 512):
        _attn_check(q, kc, vc, lens, n_tok, T, H, scale, al, tbl, window, chunk, ws, refs, f"{what} chunk={chunk}")
    n_tok = _i32((1, T - 1, 1))
    refs = _refs(q, kc, vc, lens, n_tok, T, H, scale, al, tbl, window)
    _attn_check(q, kc, vc, lens, n_tok, T, H, scale, al, tbl, window, 64, ws, refs, f"{what} n_tok=(1, T-1, 1)")
    # the same workspace with shorter lengths (every row read stays inside the planted live ranges)
    lens2, n_tok = _i32((200, 70, T - 1)), _i32((T, 1, T - 1))
    refs = _refs(q, kc, vc, lens2, n_tok, T, H, scale, al, tbl, window)
    _attn_check(q, kc, vc, lens2, n_tok, T, H, scale, al, tbl, window, 64, ws, refs, f"{what} reused workspace")


def test_spec_attention_head_dim_72():
    """D = 72 (9 of a 16-lane group's lanes hold dims) is inside the kernel's D % 8 == 0 rule."""
    q, kc, vc, tbl, H, lens = _attn_case(72, 1, 4, 16, BF16, 72)
    lens, n_tok = _i32(lens), _i32((4, 4, 4))
    refs = _refs(q, kc, vc, lens, n_tok, 4, H, 72 ** -0.5, None, tbl, 0)
    _attn_check(q, kc, vc, lens, n_tok, 4, H, 72 ** -0.5, None, tbl, 0, 64, None, refs, "D=72")


def test_spec_attention_refuses_unsupported_shapes():
    """Three query heads per KV head at head_dim 72 (6 queries), G * T = 16, T = 1 and a head_dim that is
    no multiple of 8: a nonzero status, and ``out`` is not written."""
    L = 64
    for D, Hkv, G, T in ((72, 2, 3, 2), (64, 2, 2, 8), (64, 2, 8, 2), (64, 2, 2, 1), (12, 2, 1, 2)):
        H = Hkv * G
        kc = torch.zeros(2, Hkv, L, D, dtype=BF16, device=dev)
        q = torch.randn(T, H * D, device=dev).to(BF16)
        out = torch.full((T, H * D), 5.0, device=dev, dtype=BF16)
        with pytest.raises(RuntimeError, match="kca_spec_attn returned status"):
            spec.spec_attention(q, kc, kc.clone(), _i32([0]), _i32([40]), _i32([T]), T, H, L, out=out)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())
        assert not spec.supported(D, H, Hkv, T)


# ---------------------------------------------------------------------------------------- engine
class EveryFifthWrong(Scripted):
    """``Scripted`` over the spec-off engine's greedy outputs with the draft of every fifth output
    position wrong."""

    def __init__(self, scripts):
        super().__init__(scripts, wrong=range(4, 1024, 5))


IDENTICAL: dict = {}


def _spec_engine_case(m, B, T, what, monkeypatch, arm="kernel", **kw):
    """``arm``: "kernel" -- the multi-token attention kernel whatever the bucket's size
    (KCA_DECODE_SPEC_ROWS_WORK=0) -- or "auto", the runner's own choice, which at these sizes (bf16,
    T >= 4) is the one-token kernel on B * T rows."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    if arm == "kernel":
        monkeypatch.setenv("KCA_DECODE_SPEC_ROWS_WORK", "0")
    else:
        monkeypatch.delenv("KCA_DECODE_SPEC_ROWS_WORK", raising=False)
    sp = SamplingParams(max_new_tokens=NEW, do_sample=False)
    off = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, **kw)
    rounds = [make_prompts(B, 10 * B + r) for r in range(ROUNDS[B])]
    base = [[q.output for q in off.generate(prompts, sp)] for prompts in rounds]
    assert off.stats["spec_steps"] == 0 and off.runner.spec_steps == 0
    script = EveryFifthWrong({tuple(p): o for prompts, outs in zip(rounds, base) for p, o in zip(prompts, outs)})
    eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True, spec_tokens=T, proposer=script, **kw)
    r = eng.runner
    assert r.use_graphs and r.spec_tokens == T and not eng.pipeline
    checked = total = 0
    same = True
    want_drafted = want_accepted = 0
    for prompts, outs0 in zip(rounds, base):
        outs = [q.output for q in eng.generate(prompts, sp)]
        assert all(len(o) == NEW for o in outs)
        checked += sum(check_against_forward(m, p, o) for p, o in zip(prompts, outs))
        total += NEW * B
        same = same and outs == outs0
        for p, o in zip(prompts, outs):
            _, d, a = implied(script, p, o, T, NEW)
            want_drafted, want_accepted = want_drafted + d, want_accepted + a
    st = eng.stats
    IDENTICAL[what] = same
    print(f"{what}: {checked} of {total} tokens checked; {st['spec_steps']} verify steps, {st['spec_accepted']} of "
          f"{st['spec_drafted']} drafts accepted; identical to the spec-off output: {same}; launches per verify "
          f"step {r.step_launches.get(('spec', 1 if B == 1 else 4, T))}")
    assert 2 * checked >= total
    assert st["spec_steps"] > 0 and st["spec_accepted"] >= 1 and r.spec_steps > 0
    assert r.spec_rows_steps == (0 if arm == "kernel" else r.spec_steps)
    assert any(k[0] == "spec" for k in r._graphs if isinstance(k, tuple))
    assert st["decode_tokens"] == (NEW - 1) * B * len(rounds)
    # the counts the script implies for the outputs the engine produced (whatever they are) ...
    assert (st["spec_drafted"], st["spec_accepted"]) == (want_drafted, want_accepted)
    if same:  # ... which, where the output is the spec-off output, is the scripted count itself
        n = sum(implied(script, p, o, T, NEW)[2] for prompts, outs in zip(rounds, base) for p, o in zip(prompts, outs))
        assert st["spec_accepted"] == n
    prompts = make_prompts(B, 10 * B)
    sp = SamplingParams(max_new_tokens=10, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
    a = [q.output for q in eng.generate(prompts, sp)]
    b = [q.output for q in eng.generate(prompts, sp)]
    assert a == b and all(len(x) == 10 for x in a)
    c = [q.output for q in off.generate(prompts, sp)]
    print(f"{what}: seeded sampled output identical to the spec-off engine's: {a == c}")
    return eng


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [1, 3])
def test_engine_spec(preset, B, monkeypatch):
    """Draft and verify behind HIP graphs, T = 4: every generated token whose top-2 margin in the model's
    own full forward is clear is that forward's argmax, at least half are clear, verify steps ran and
    accepted drafts, the accepted / drafted counts are the ones the script implies, and a seeded sampled
    run replays bit-identically (also on a second ``generate`` of the same engine)."""
    _spec_engine_case(small_lm(preset), B, 4, f"{preset} B={B} T=4", monkeypatch)


@pytest.mark.parametrize("preset,B", [("gpt-j-6b", 3), ("bloom-560m", 1), ("gpt-neox-20b", 3)])
def test_engine_spec_short_stream_arm(preset, B, monkeypatch):
    """The runner's own dispatch at these sizes: kca_spec_prep + the one-token attention kernel on the
    B * T rows (engine/runner.py ``_spec_rows``). The same checks."""
    _spec_engine_case(small_lm(preset), B, 4, f"{preset} B={B} T=4 rows arm", monkeypatch, arm="auto")


@pytest.mark.parametrize("T", [2, 8])
def test_engine_spec_other_T(T, monkeypatch):
    _spec_engine_case(small_lm("gpt-j-6b"), 3, T, f"gpt-j-6b B=3 T={T}", monkeypatch)


def test_engine_spec_fp16_model(monkeypatch):
    _spec_engine_case(small_lm("gpt-j-6b", dtype=F16), 3, 4, "gpt-j-6b fp16 B=3 T=4", monkeypatch)


def test_engine_spec_fp8_weights(monkeypatch):
    eng = _spec_engine_case(small_lm("gpt-j-6b"), 3, 4, "gpt-j-6b fp8 weights B=3 T=4", monkeypatch,
                            weight_dtype="fp8")
    assert eng.runner.w8_steps > 0 and eng.runner.batched_steps == 0


def test_engine_spec_mxfp4_weights(monkeypatch):
    from .test_mx4_gpu import small_lm as small_lm_mx4
    eng = _spec_engine_case(small_lm_mx4("gpt-j-6b"), 3, 4, "gpt-j-6b mxfp4 weights B=3 T=4", monkeypatch,
                            weight_dtype="mxfp4")
    assert eng.runner.mx4_steps > 0 and eng.runner.batched_steps == 0


def test_engine_spec_identical_cases_report():
    """Which engine cases of this run produced the spec-off output token for token (printed, not required:
    the verify step's M = B * T rows take other kernels than a B-row decode step, and a near-tie may fall
    the other way)."""
    print("identical to the spec-off output:", {k: v for k, v in IDENTICAL.items()} or "no engine case ran")
