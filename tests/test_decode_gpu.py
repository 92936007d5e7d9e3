"""Decode kernels (kca_decode_prep / kca_decode_attn / kca_sample_logits) vs
fp32 PyTorch references, and the engine's graph-captured decode on MI355X."""
import math

import pytest
import torch
import torch.nn.functional as F

from kubernetes_cloud_amd.ops import _lib
from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops.rope import rope_tables

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


@pytest.mark.parametrize("D,rot,inter", [(256, 64, True), (96, 24, False), (80, 20, False), (64, 0, False),
                                         (128, 128, False)])
def test_decode_prep(D, rot, inter):
    torch.manual_seed(0)
    B, H, Hkv, S, L = 5, 4, 4, 7, 64
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
    pos = torch.tensor([0, 3, 63, 17, 5], device=dev, dtype=torch.int32)
    slots = torch.tensor([6, 0, 2, 3, 1], device=dev, dtype=torch.int32)
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    kc = torch.zeros(S, Hkv, L, D, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q2, kc2, vc2 = qkv.cpu().float(), kc.cpu().float(), vc.cpu().float()
    dops.decode_prep(qkv, H, Hkv, D, rot, inter, cos, sin, pos, slots, kc, vc)
    dops.decode_prep(q2, H, Hkv, D, rot, inter, cos.cpu() if rot else None, sin.cpu() if rot else None,
                     pos.cpu(), slots.cpu(), kc2, vc2)
    torch.cuda.synchronize()
    assert (qkv.cpu().float() - q2).abs().max() < 2e-2
    assert (kc.cpu().float() - kc2).abs().max() < 2e-2
    assert torch.equal(vc.cpu().float(), vc2)


@pytest.mark.parametrize("D", [64, 80, 96, 128, 256])
@pytest.mark.parametrize("G", [1, 4])
def test_decode_attention(D, G):
    torch.manual_seed(D + G)
    B, Hkv, L = 6, 4, 2048
    H = Hkv * G
    kc = torch.randn(B + 1, Hkv, L, D, device=dev).to(torch.bfloat16)
    vc = torch.randn_like(kc)
    q = torch.randn(B, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
    slots = torch.tensor([3, 0, 6, 1, 2, 5], device=dev, dtype=torch.int32)
    lens = torch.tensor([1, 2048, 700, 65, 1500, 129], device=dev, dtype=torch.int32)
    alibi = None
    for max_kv, chunk in ((2048, 0), (2048, 32), (2048, 64), (2048, 1024)):  # short (two-phase) and online
        o = dops.decode_attention(q, kc, vc, slots, lens, H, max_kv, chunk=chunk)
        ref = dops.decode_attention_reference(q.float(), kc.float(), vc.float(), slots, lens, H,
                                              1 / math.sqrt(D), alibi, torch.empty(B, H * D, device=dev))
        assert (o.float() - ref).abs().max() < 2e-2, (max_kv, chunk)


def test_decode_attention_alibi():
    torch.manual_seed(1)
    B, H, D, L = 3, 8, 128, 512
    from kubernetes_cloud_amd.models.causal_lm import alibi_slopes
    al = alibi_slopes(H).to(dev)
    kc = torch.randn(B, H, L, D, device=dev).to(torch.bfloat16)
    vc = torch.randn_like(kc)
    q = torch.randn(B, 3 * H * D, device=dev).to(torch.bfloat16)
    slots = torch.arange(B, device=dev, dtype=torch.int32)
    lens = torch.tensor([512, 100, 301], device=dev, dtype=torch.int32)
    o = dops.decode_attention(q, kc, vc, slots, lens, H, 512, alibi=al)
    ref = dops.decode_attention_reference(q.float(), kc.float(), vc.float(), slots, lens, H, 1 / math.sqrt(D),
                                          al, torch.empty(B, H * D, device=dev))
    assert (o.float() - ref).abs().max() < 2e-2


def _params(B, t, k, p, r=1.0):
    f = lambda v, dt: torch.full((B,), v, dtype=dt, device=dev)  # noqa: E731
    return dict(temperature=f(t, torch.float32), top_k=f(k, torch.int32), top_p=f(p, torch.float32),
                rep_penalty=f(r, torch.float32))


@pytest.mark.parametrize("V", [50400, 250880, 1000])
def test_sample_greedy_and_masks(V):
    torch.manual_seed(0)
    B = 8
    logits = (torch.randn(B, V, device=dev) * 4).to(torch.bfloat16)
    ids, lp = dops.sample_logits(logits, **_params(B, 0.0, 0, 1.0))
    ref = logits.float().argmax(-1)
    assert torch.equal(ids, ref)
    assert torch.allclose(lp, torch.log_softmax(logits.float(), -1).gather(1, ref[:, None])[:, 0], atol=1e-3)
    # kept-set sizes of the top-k / top-p radix selects == HF warper masks
    for (t, k, p) in ((1.0, 50, 1.0), (0.7, 0, 0.9), (1.3, 40, 0.8), (1.0, 1, 1.0), (1.0, 0, 0.5)):
        kept = torch.empty(B, dtype=torch.int32, device=dev)
        ids, _ = dops.sample_logits(logits, **_params(B, t, k, p), seeds=torch.arange(B, device=dev),
                                    out_kept=kept)
        x = logits.float() / t
        for b in range(B):
            keep = dops.keep_mask_reference(x[b], k, p)
            # the kernel keeps every token tied with the threshold value (bf16 logits tie often);
            # HF's sort keeps an arbitrary subset of a tie group at the top-p cut
            expect = int((x[b] >= x[b][keep].min()).sum())
            assert int(keep.sum()) <= int(kept[b]) <= expect + max(1, expect // 100), (t, k, p, b)
            assert bool(keep[ids[b]]), (t, k, p, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_sample_topk_topp_distribution(dtype):
    """Top-k + top-p sampling draws from the renormalised kept set: fp32 logits take the memory-pass
    kernel (top-k survivors compacted in LDS), bf16 the register-resident one."""
    torch.manual_seed(1)
    V, B, k, p = 3000, 8192, 12, 0.9
    base = (torch.randn(V, device=dev) * 2).to(dtype).float()
    logits = base[None].expand(B, V).contiguous().to(dtype)
    seeds = torch.randint(0, 2**62, (B,), device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ids, lp = dops.sample_logits(logits, **_params(B, 1.0, k, p), seeds=seeds, out_kept=kept)
    keep = dops.keep_mask_reference(base.float(), k, p)
    assert bool(keep[ids].all())
    assert int(kept[0]) == int(keep.sum())
    probs = torch.where(keep, base.float(), torch.full_like(base, -float("inf"))).softmax(-1)
    freq = torch.bincount(ids, minlength=V).float() / B
    assert (freq - probs).abs().max() < 0.03
    ref_lp = torch.log_softmax(base.float(), -1)[ids]
    assert torch.allclose(lp, ref_lp, atol=1e-3)


@pytest.mark.parametrize("V", [1000, 50400])
def test_sample_register_kernel_penalty_bans(V):
    """bf16 logits (the register-resident sampler): repetition penalty through the seen mask and
    banned ids match the reference for greedy picks, top-k kept counts match HF masks."""
    torch.manual_seed(3)
    B = 4
    logits = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16)
    top = logits.float().argmax(-1)
    seen = torch.zeros(B, V, dtype=torch.uint8, device=dev)
    seen[0, top[0]] = 1
    seen[2, top[2]] = 1
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    bans = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    bans[1, 0] = top[1]
    bans[3, 1] = top[3]
    ref = dops.sample_logits_reference(logits.float().cpu(), *(v.cpu() for v in _params(B, 0.0, 0, 1.0, 30.0).values()),
                                       seen=seen.cpu().clone(), slots=slots.cpu(), ban_ids=bans.cpu())[0]
    ids, lp = dops.sample_logits(logits, **_params(B, 0.0, 0, 1.0, 30.0), seen=seen.clone(), slots=slots,
                                 ban_ids=bans)
    assert ids.tolist() == ref.tolist()
    assert all(int(ids[b]) != int(top[b]) for b in range(B))
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ids, _ = dops.sample_logits(logits, **_params(B, 0.8, 40, 1.0), seeds=torch.arange(B, device=dev), out_kept=kept)
    for b in range(B):
        keep = dops.keep_mask_reference(logits[b].float() / 0.8, 40, 1.0)
        expect = int((logits[b].float() / 0.8 >= (logits[b].float() / 0.8)[keep].min()).sum())
        assert int(keep.sum()) <= int(kept[b]) <= expect and bool(keep[ids[b]])


def test_sample_penalty_bans_distribution():
    torch.manual_seed(0)
    V = 64
    base = torch.randn(V, device=dev)
    B = 4096
    logits = base[None].expand(B, V).contiguous()
    seeds = torch.randint(0, 2**62, (B,), device=dev)
    ids, _ = dops.sample_logits(logits, **_params(B, 1.0, 0, 1.0), seeds=seeds)
    freq = torch.bincount(ids, minlength=V).float() / B
    probs = base.softmax(-1)
    assert (freq - probs).abs().max() < 0.03
    # repetition penalty through the seen mask + bans
    seen = torch.zeros(2, V, dtype=torch.uint8, device=dev)
    top = int(base.argmax())
    seen[0, top] = 1
    slots = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    bans = torch.tensor([[-1], [top]], dtype=torch.int32, device=dev)
    x = base[None].expand(2, V).contiguous()
    ref = dops.sample_logits_reference(x.cpu(), *(v.cpu() for v in _params(2, 0.0, 0, 1.0, 50.0).values()),
                                       seen=seen.cpu().clone(), slots=slots.cpu(), ban_ids=bans.cpu())[0]
    ids, _ = dops.sample_logits(x, **_params(2, 0.0, 0, 1.0, 50.0), seen=seen, slots=slots, ban_ids=bans)
    assert ids.tolist() == ref.tolist() and top not in ids.tolist()
    assert int(seen[1, ids[1]]) == 1  # chosen token is marked seen


@pytest.mark.parametrize("preset", ["gpt-j-6b", "bloom-560m", "gpt2"])
def test_engine_gpu_graphs_match_eager_and_recompute(preset):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    small = {"gpt-j-6b": dict(n_embd=1024, n_layer=2, n_head=4, rotary_dim=64, n_positions=512),
             "bloom-560m": dict(hidden_size=512, n_layer=2, n_head=4),
             "gpt2": dict(n_embd=512, n_layer=2, n_head=8, n_positions=512)}[preset]
    cfg = dict(PRESETS_HF[preset])
    cfg.update(small)
    m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)
    prompts = [[int(x) for x in torch.randint(0, 1000, (n,))] for n in (5, 33, 5, 100)]
    sp = SamplingParams(max_new_tokens=12, do_sample=False)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(m, max_slots=8, max_len=256, use_graphs=graphs)
        outs.append([r.output for r in eng.generate(prompts, sp)])
    assert outs[0] == outs[1]
    # every generated token is the argmax of a full forward (except near-ties)
    for p, o in zip(prompts, outs[1]):
        with torch.no_grad():
            lg = m(torch.tensor([p + o], device=dev))[0].float()
        for i, t in enumerate(o):
            row = lg[len(p) - 1 + i]
            top2 = row.topk(2).values
            if float(top2[0] - top2[1]) > 0.1:
                assert int(row.argmax()) == t, (preset, i)
    # seeded sampling is reproducible under graphs
    eng = LLMEngine(m, max_slots=8, max_len=256, use_graphs=True)
    sp2 = SamplingParams(max_new_tokens=16, temperature=0.9, top_k=40, top_p=0.95, seed=7)
    a = [r.output for r in eng.generate(prompts, sp2)]
    b = [r.output for r in eng.generate(prompts, sp2)]
    assert a == b
    assert _lib.has("kca_decode_attn")


@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("N,K", [(4096, 4096), (12288, 4096), (4096, 16384), (5376, 14336), (14336, 1792)])
def test_skinny_gemm(M, N, K):
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=dev).to(torch.bfloat16)
    ref = x.float() @ w.float().t() + b.float()
    for act, fn in ((0, lambda t: t), (1, lambda t: torch.nn.functional.gelu(t, approximate="tanh")),
                    (2, torch.nn.functional.gelu)):
        y = skinny_linear(x, w, b, act)
        assert y.shape == (M, N)
        assert (y.float() - fn(ref)).abs().max() < 0.05, act


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("N,K", [(12288, 4096), (4098, 4096), (4096, 16384), (1026, 1000)])
def test_skinny_gemm_multirow_kernel(M, N, K):
    """kca_skinny_gemm at 2-4 rows (the K-split register-resident kernel for K <= 8192, the
    row-per-wave kernel beyond), called directly: skinny_linear sends these shapes to hipBLASLt
    unless KCA_SKINNY_MAX_M says otherwise. Strided x / y rows, ragged N, bias + GELU."""
    torch.manual_seed(M * 7 + N + K)
    xs = torch.randn(M, K + 8, device=dev).to(torch.bfloat16)
    x = xs[:, :K]
    w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=dev).to(torch.bfloat16)
    ys = torch.full((M, N + 4), float("nan"), device=dev, dtype=torch.bfloat16)
    y = ys[:, :N]
    _lib.call("kca_skinny_gemm", x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), y.data_ptr(), y.stride(0),
              M, N, K, 1, _lib.stream())
    torch.cuda.synchronize()
    ref = torch.nn.functional.gelu(x.float() @ w.float().t() + b.float(), approximate="tanh")
    assert (y.float() - ref).abs().max() < 0.05
    assert torch.isnan(ys[:, N:].float()).all()  # nothing written past the row


@pytest.mark.parametrize("M", [1, 2, 4])
def test_skinny_gemm_row_per_wave_kernel(M):
    """The row-per-wave skinny kernel (A/B alternative to the split-K default)."""
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    torch.manual_seed(M)
    x = torch.randn(M, 4096, device=dev).to(torch.bfloat16)
    w = (torch.randn(2048, 4096, device=dev) * 0.02).to(torch.bfloat16)  # small: skinny for every M <= 4
    ref = x.float() @ w.float().t()
    _lib.call("kca_skinny_set_splitk", 0)
    try:
        y = skinny_linear(x, w)
    finally:
        _lib.call("kca_skinny_set_splitk", 1)
    assert (y.float() - ref).abs().max() < 0.05
    assert (skinny_linear(x, w).float() - ref).abs().max() < 0.05


_LN_SKINNY_SHAPES = [(1, 12288, 4096), (2, 4096, 4096), (4, 4096, 4096), (1, 5376, 14336), (2, 1024, 14336),
                     (3, 4096, 4096)]
# every (split, nres, shape) except split with M != 1: the split path is M == 1 only
_LN_SKINNY_CASES = [(M, N, K, nres, split) for split in (False, True) for nres in (0, 1, 2)
                    for (M, N, K) in _LN_SKINNY_SHAPES if not (split and M != 1)]


@pytest.mark.parametrize("M,N,K,nres,split", _LN_SKINNY_CASES,
                         ids=[f"{c[4]}-{c[3]}-{c[0]}-{c[1]}-{c[2]}" for c in _LN_SKINNY_CASES])
def test_ln_skinny_gemm(M, N, K, nres, split, monkeypatch):
    """split: at M = 1 the LN runs once (kca_ln_rows) before the plain GEMV;
    otherwise every GEMV workgroup normalises its activation slice itself."""
    from kubernetes_cloud_amd.ops import gemv
    monkeypatch.setattr(gemv, "_LN_SPLIT_M1", split)
    torch.manual_seed(M * 7 + N + K + nres)
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    res = tuple(torch.randn(M, K, device=dev).to(torch.bfloat16) for _ in range(nres))
    g = (1 + 0.1 * torch.randn(K, device=dev)).to(torch.bfloat16)
    be = (0.1 * torch.randn(K, device=dev)).to(torch.bfloat16) if nres != 1 else None
    w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=dev).to(torch.bfloat16)
    assert gemv._ln_ok(x, M, K, w, res, g, be, b)  # the fused kernel, not the fallback, is under test
    hs = x.float()
    for r in res:
        hs = hs + r.float()
    h_ref = hs.to(torch.bfloat16)
    xn = torch.nn.functional.layer_norm(h_ref.float(), (K,), g.float(), None if be is None else be.float(), 1e-5)
    ref = xn.to(torch.bfloat16).float() @ w.float().t() + b.float()
    y, h, xo = gemv.ln_skinny_linear(x, g, be, 1e-5, w, b, res, act=1, want_xn=True)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref)
    assert (xo.float() - xn).abs().max() < 0.05  # normalised rows (GPT-J shared-LN output)
    assert (y.float() - torch.nn.functional.gelu(ref, approximate="tanh")).abs().max() < 0.06


def test_dalle_mini_predictor_on_gpu():
    """S12 on the MI355X path (bf16, flash attention, NHWC VQGAN decoder): PNG out,
    deterministic per seed."""
    import io as _io

    from tests.test_serving_cpu import _tiny_dalle_cfgs
    from kubernetes_cloud_amd.serving.dalle_service import DalleMiniPredictor, options
    c, v = _tiny_dalle_cfgs()
    p = DalleMiniPredictor("dalle-mini", None, options({}), device=torch.device("cuda", 0), config=c, vq_config=v)
    p.load()
    a = p.predict({"prompt": "a red fox", "parameters": {"seed": 3, "top_k": 8}})
    b = p.predict({"prompt": "a red fox", "parameters": {"seed": 3, "top_k": 8}})
    from PIL import Image
    assert a[:8] == b"\x89PNG\r\n\x1a\n" and a == b
    assert Image.open(_io.BytesIO(a)).size == (8, 8)


def _paginate(kc, PS, seed=0):
    """Contiguous [S, Hkv, L, D] -> (shuffled page pool [S*L/PS + 1, Hkv, PS, D], block table [S, L/PS])."""
    S, Hkv, L, D = kc.shape
    nb = L // PS
    perm = torch.randperm(S * nb, generator=torch.Generator().manual_seed(seed))
    pool = torch.zeros(S * nb + 1, Hkv, PS, D, device=kc.device, dtype=kc.dtype)
    pages = kc.view(S, Hkv, nb, PS, D).permute(0, 2, 1, 3, 4).reshape(S * nb, Hkv, PS, D)
    pool[perm.to(kc.device)] = pages
    return pool, perm.view(S, nb).to(torch.int32).to(kc.device)


@pytest.mark.parametrize("D,G,PS", [(256, 1, 64), (128, 4, 16), (80, 1, 256), (64, 2, 32)])
def test_decode_attention_paged_equals_contiguous(D, G, PS):
    torch.manual_seed(D + G)
    B, Hkv, L = 6, 4, 2048
    H = Hkv * G
    kc = torch.randn(B + 1, Hkv, L, D, device=dev).to(torch.bfloat16)
    vc = torch.randn_like(kc)
    kp, tbl = _paginate(kc, PS, 1)
    vp, _ = _paginate(vc, PS, 1)
    q = torch.randn(B, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
    slots = torch.tensor([3, 0, 6, 1, 2, 5], device=dev, dtype=torch.int32)
    lens = torch.tensor([1, 2048, 700, 65, 1500, 129], device=dev, dtype=torch.int32)
    for chunk in (0, 32, 64, 1024):
        a = dops.decode_attention(q, kc, vc, slots, lens, H, L, chunk=chunk)
        b = dops.decode_attention(q, kp, vp, slots, lens, H, L, chunk=chunk, block_table=tbl)
        assert torch.equal(a, b), chunk  # same values, same reduction order
    ref = dops.decode_attention_reference(q.float(), kp.float(), vp.float(), slots, lens, H, 1 / math.sqrt(D),
                                          None, torch.empty(B, H * D, device=dev), tbl)
    assert (b.float() - ref).abs().max() < 2e-2


def test_decode_prep_paged_equals_contiguous():
    torch.manual_seed(0)
    B, H, Hkv, D, S, L, PS = 5, 4, 4, 256, 7, 256, 64
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
    pos = torch.tensor([0, 3, 255, 64, 130], device=dev, dtype=torch.int32)
    slots = torch.tensor([6, 0, 2, 3, 1], device=dev, dtype=torch.int32)
    cos, sin = rope_tables(64, L, 10000.0, dev)
    kc = torch.zeros(S, Hkv, L, D, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    kp, tbl = _paginate(kc, PS, 2)
    vp, _ = _paginate(vc, PS, 2)
    q1, q2 = qkv.clone(), qkv.clone()
    dops.decode_prep(q1, H, Hkv, D, 64, True, cos, sin, pos, slots, kc, vc)
    dops.decode_prep(q2, H, Hkv, D, 64, True, cos, sin, pos, slots, kp, vp, block_table=tbl)
    assert torch.equal(q1, q2)
    for s in range(S):
        assert torch.equal(dops.gather_kv(kp, s, L, tbl), kc[s]) and torch.equal(dops.gather_kv(vp, s, L, tbl), vc[s])


def _gpu_model(preset):
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    small = {"gpt-j-6b": dict(n_embd=1024, n_layer=2, n_head=4, rotary_dim=64, n_positions=512),
             "bloom-560m": dict(hidden_size=512, n_layer=2, n_head=4)}[preset]
    cfg = dict(PRESETS_HF[preset])
    cfg.update(small)
    return build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)


@pytest.mark.parametrize("preset", ["gpt-j-6b", "bloom-560m"])
def test_engine_gpu_paged_and_ragged(preset):
    """Paged cache == contiguous cache exactly; mixed prompt lengths prefilled in
    one ragged batch == each prompt run alone (up to bf16 near-ties of the
    batched vs single-row GEMMs); beam search paged == contiguous."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = _gpu_model(preset)
    g = torch.Generator().manual_seed(1)
    prompts = [[int(x) for x in torch.randint(0, 1000, (n,), generator=g)] for n in (7, 150, 33, 64, 1, 90)]
    sp = SamplingParams(max_new_tokens=20, do_sample=False)
    runs = {}
    for ps in (0, 16, 64):
        eng = LLMEngine(m, max_slots=8, max_len=256, page_size=ps)
        runs[ps] = [r.output for r in eng.generate(prompts, sp)]
        assert eng.stats["prefill_batches"] < len(prompts)
        if ps:
            assert eng.runner.cache.free_count() == eng.runner.cache.n_pages
    assert runs[0] == runs[16] == runs[64]
    for p, o in zip(prompts, runs[64]):
        solo = LLMEngine(m, max_slots=1, max_len=256).generate([p], sp)[0].output
        i = next((j for j, (a, b) in enumerate(zip(o, solo)) if a != b), None)
        if i is not None:  # allowed only where the two best logits are within bf16 noise
            with torch.no_grad():
                row = m(torch.tensor([p + o[:i]], device=dev))[0, -1].float()
            top2 = row.topk(2).values
            assert float(top2[0] - top2[1]) < 0.1, (preset, len(p), i)
    beams = [LLMEngine(m, max_slots=4, max_len=256, page_size=ps).beam_generate(
        prompts[2], num_beams=4, max_new_tokens=16, n_return=4).sequences for ps in (0, 16)]
    assert beams[0] == beams[1]


def test_layer_split_gpu_cpu_engine(tmp_path):
    """PAR-9 fallback: a model split over the MI355X and host memory serves
    through the engine (per-layer KV caches on each layer's device) and its
    prefill logits match the all-GPU model."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.io.hf import load_pretrained
    from kubernetes_cloud_amd.parallel import layer_split as ls

    from .helpers import make_model_dir
    d = make_model_dir(str(tmp_path / "m"), "gpt-j-6b", n_embd=256, n_layer=4, n_head=4, rotary_dim=32,
                       vocab_size=512, tokenizer=False)
    full = load_pretrained(d, device=dev, dtype=torch.bfloat16)
    meta_blk = ls._nbytes(full.h[0], torch.bfloat16)
    emb = ls._nbytes(full.wte, torch.bfloat16)
    m = ls.load_layer_split(d, {0: emb + 2 * meta_blk + 1024, "cpu": 1 << 30}, dtype=torch.bfloat16)
    assert m.hf_device_map["h.1"].startswith("cuda") and m.hf_device_map["h.2"] == "cpu"
    eng = LLMEngine(m, max_slots=2, max_len=64)
    r = eng.runner
    assert r.multi_device and r.cache.k[0].is_cuda and not r.cache.k[3].is_cuda
    ids = torch.tensor([[5, 9, 2, 7, 1, 3]])
    a = r.prefill(ids, [0]).float()
    b = LLMEngine(full, max_slots=2, max_len=64).runner.prefill(ids, [0]).float()
    assert (a - b).abs().max() < 0.1 * b.abs().max()
    out = eng.generate([[5, 9, 2], [1, 2, 3, 4, 5]], SamplingParams(max_new_tokens=6, do_sample=False))
    assert all(len(x.output) == 6 for x in out)


@pytest.mark.parametrize("D,rot,inter,G,PS", [(256, 64, True, 1, 64), (256, 64, True, 1, 0), (128, 32, False, 4, 16),
                                              (80, 20, False, 1, 0), (64, 0, False, 2, 32)])
@pytest.mark.parametrize("CH", [0, 128])
def test_decode_prep_attention_fused_equals_two_kernels(D, rot, inter, G, PS, CH, monkeypatch):
    """kca_decode_prep_attn (one launch) == kca_decode_prep + kca_decode_attn, bit for bit:
    same rotated Q, same appended K/V rows, same attention output (CH 128: the one-pass
    online-softmax kernel, which folds the last token in after its loop in both modes)."""
    if CH:
        monkeypatch.setattr(dops, "decode_chunk", lambda *a: CH)
    torch.manual_seed(D + rot + G)
    B, Hkv, L = 5, 4, 512
    H = Hkv * G
    kc = torch.randn(B + 1, Hkv, L, D, device=dev).to(torch.bfloat16)
    vc = torch.randn_like(kc)
    tbl = None
    if PS:
        kc, tbl = _paginate(kc, PS, 3)
        vc, _ = _paginate(vc, PS, 3)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
    slots = torch.tensor([3, 0, 5, 1, 2], device=dev, dtype=torch.int32)
    pos = torch.tensor([0, 511, 200, 63, 64], device=dev, dtype=torch.int32)
    kl = pos + 1
    cos, sin = rope_tables(rot, L, 10000.0, dev) if rot else (None, None)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    q1, q2 = qkv.clone(), qkv.clone()
    dops.decode_prep(q1, H, Hkv, D, rot, inter, cos, sin, pos, slots, k1, v1, block_table=tbl)
    a = dops.decode_attention(q1, k1, v1, slots, kl, H, L, block_table=tbl, chunk=CH)
    b = dops.decode_prep_attention(q2, H, Hkv, D, rot, inter, cos, sin, pos, slots, k2, v2, kl, L, block_table=tbl)
    torch.cuda.synchronize()
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert torch.equal(a, b)
    assert torch.equal(q2, qkv)  # the fused kernel leaves the QKV buffer untouched


_FANIN_CASE = """
import sys, torch
from kubernetes_cloud_amd.ops import decode as dops
torch.manual_seed(7)
dev = torch.device("cuda", 0)
B, Hkv, G, D, L = 3, 4, 4, 128, 2048
kc = torch.randn(B, Hkv, L, D, device=dev).to(torch.bfloat16)
vc = torch.randn_like(kc)
q = torch.randn(B, (Hkv * G + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
slots = torch.tensor([2, 0, 1], device=dev, dtype=torch.int32)
lens = torch.tensor([2048, 33, 1000], device=dev, dtype=torch.int32)
outs = [dops.decode_attention(q, kc, vc, slots, lens, Hkv * G, L, chunk=c).cpu() for c in (32, 64, 256, 0)]
torch.save(outs, sys.argv[1])
"""


def test_decode_split_fanin_matches_combine_kernel(tmp_path):
    """The split-K fan-in (last split's workgroup combines, csrc/kernels/decode.hip
    fanin_combine) is bit-identical to the separate combine kernel (KCA_DECODE_FANIN=0)
    at 64 / 32 / 8 splits and the default split policy."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for f in ("1", "0"):
        out = str(tmp_path / f"o{f}.pt")
        env = dict(os.environ, KCA_DECODE_FANIN=f, PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", _FANIN_CASE, out], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[f] = torch.load(out, weights_only=True)
    for a, b in zip(res["1"], res["0"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("preset", ["gpt-j-6b", "bloom-560m"])
def test_engine_gpu_chunked_prefill(preset):
    """Chunked prefill on the GPU (prefill continuation through the HIP flash
    kernel with Sk > Sq, bottom-right causal; paged KV): a 300-token prompt
    admitted while a stream decodes is prefilled 64 tokens per step, the
    stream advances every step, and the outputs equal the unchunked engine
    (up to bf16 near-ties: chunked and one-pass prefill run different GEMM shapes)."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = _gpu_model(preset)
    g = torch.Generator().manual_seed(2)
    short = [int(x) for x in torch.randint(0, 1000, (9,), generator=g)]
    long = [int(x) for x in torch.randint(0, 1000, (300,), generator=g)]
    sp = SamplingParams(max_new_tokens=16, do_sample=False)
    eng = LLMEngine(m, max_slots=4, max_len=400, prefill_chunk=64)
    r1 = eng.add_request(short, SamplingParams(max_new_tokens=40, do_sample=False))
    eng.step()
    r2 = eng.add_request(long, sp)
    steps = 0
    while not r2.output:
        before = len(r1.output)
        eng.step()
        steps += 1
        assert len(r1.output) == before + 1
    assert steps >= 300 // 64 and eng.stats["max_step_prefill_tokens"] <= 64
    eng.run_until_done([r1, r2])
    ref = LLMEngine(m, max_slots=4, max_len=400).generate([long], sp)[0].output
    i = next((j for j, (a, b) in enumerate(zip(r2.output, ref)) if a != b), None)
    if i is not None:
        with torch.no_grad():
            row = m(torch.tensor([long + ref[:i]], device=dev))[0, -1].float()
        top2 = row.topk(2).values
        assert float(top2[0] - top2[1]) < 0.1, (preset, i)


@pytest.mark.parametrize("N,K1,K2,two_ln", [(4096, 4096, 16384, False), (6144, 6144, 24576, True),
                                             (14336, 1792, 0, False), (14336, 7168, 0, True)])
def test_gemv_dual_ln_matches_reference(N, K1, K2, two_ln):
    """decode.hip gemv_dual_ln_kernel: y = x1 W1^T (+ x2 W2^T) + b, h' = h + y, LN(h') in one launch
    (arrival counter, last workgroup normalises) -- GPT-J (two weight streams), GPT-NeoX-20B (two
    LayerNorms of h'), BLOOM TP=8 rank shapes (one stream, N = 14336); repeated launches reuse the
    re-armed counter."""
    torch.manual_seed(3)
    bf = dict(device=dev, dtype=torch.bfloat16)
    x1 = torch.randn(1, K1, **bf)
    w1 = torch.randn(N, K1, **bf) * K1 ** -0.5
    x2 = torch.randn(1, K2, **bf) if K2 else None
    w2 = torch.randn(N, K2, **bf) * K2 ** -0.5 if K2 else None
    b, h = torch.randn(N, **bf), torch.randn(1, N, **bf)
    gamma, beta = torch.randn(N, **bf), torch.randn(N, **bf)
    g2, b2 = torch.randn(N, **bf), torch.randn(N, **bf)
    ypart = torch.empty(N, device=dev, dtype=torch.float32)
    cnt = torch.zeros(32 * 65, device=dev, dtype=torch.int32)
    hn_ref, xn_ref = dops.gemv_dual_ln_reference(x1, w1, x2, w2, b, h, gamma, beta, 1e-5)
    xn2_ref = F.layer_norm(hn_ref.float(), (N,), g2.float(), b2.float(), 1e-5)
    for _ in range(3):
        h_out, xn, xn2 = torch.empty(1, N, **bf), torch.empty(1, N, **bf), torch.empty(1, N, **bf)
        dops.gemv_dual_ln(x1, w1, x2, w2, b, h, gamma, beta, 1e-5, ypart, cnt, h_out, xn,
                          *((g2, b2, xn2) if two_ln else (None, None, None)))
        torch.cuda.synchronize()
        assert (h_out.float() - hn_ref.float()).abs().max() < 0.05
        assert (xn.float() - xn_ref).abs().max() < 0.08
        if two_ln:
            assert (xn2.float() - xn2_ref).abs().max() < 0.08
    assert int(cnt.abs().sum()) == 0  # every counter re-armed


@pytest.mark.parametrize("PS", [0, 64])
@pytest.mark.parametrize("L0", [40, 600])
def test_decode_attention_gemv_fused_matches_separate(PS, L0):
    """decode_attn_gemv_kernel: the fused prep + split-K attention workgroups give exactly the
    decode_prep_attention output and cache append, the GEMV workgroups skinny_linear's values."""
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    torch.manual_seed(5 + L0)
    H, D, rot, L = 16, 256, 64, 1024
    bf = dict(device=dev, dtype=torch.bfloat16)
    kc0 = torch.randn(2, H, L, D, device=dev).to(torch.bfloat16)
    vc0 = torch.randn_like(kc0)
    tbl = None
    if PS:
        kc0, tbl = _paginate(kc0, PS, 3)
        vc0, _ = _paginate(vc0, PS, 3)
    qkv = torch.randn(1, 3 * H * D, **bf)
    cos, sin = rope_tables(rot, L, 10000.0, dev)
    slots = torch.tensor([1], device=dev, dtype=torch.int32)
    pos = torch.tensor([L0 - 1], device=dev, dtype=torch.int32)
    kv_lens = pos + 1
    gx, gw, gb = torch.randn(1, 4096, **bf), torch.randn(16384, 4096, **bf) * 0.02, torch.randn(16384, **bf)
    ws = torch.zeros(max(dops.decode_ws_floats(1, H, H, D, L), 1), device=dev, dtype=torch.float32)
    res = []
    for fused in (False, True):
        kc, vc, out = kc0.clone(), vc0.clone(), torch.empty(1, H * D, **bf)
        if fused:
            gy = torch.empty(1, 16384, **bf)
            assert dops.decode_prep_attention_gemv(qkv.clone(), H, H, D, rot, True, cos, sin, pos, slots, kc, vc,
                                                   kv_lens, L, D ** -0.5, None, out, ws, tbl, 0, gx, gw, gb, gy, 1)
        else:
            dops.decode_prep_attention(qkv.clone(), H, H, D, rot, True, cos, sin, pos, slots, kc, vc, kv_lens, L,
                                       D ** -0.5, None, out=out, ws=ws, block_table=tbl)
            gy = skinny_linear(gx, gw, gb, 1)
        torch.cuda.synchronize()
        res.append((out, gy, kc, vc))
    (o0, y0, k0, v0), (o1, y1, k1, v1) = res
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert torch.equal(o0, o1)
    assert (y0.float() - y1.float()).abs().max() < 0.02


@pytest.mark.parametrize("PS", [0, 64])
@pytest.mark.parametrize("L0", [40, 600])
def test_decode_attention_gemv_step_descriptors(PS, L0):
    """by_row descriptors (the step's RoPE row and page row at fixed addresses, uploaded with the step
    inputs) give exactly the table-lookup path's attention output and cache append."""
    torch.manual_seed(3 + L0)
    H, D, rot, L = 16, 256, 64, 1024
    bf = dict(device=dev, dtype=torch.bfloat16)
    kc0 = torch.randn(2, H, L, D, device=dev).to(torch.bfloat16)
    vc0 = torch.randn_like(kc0)
    tbl = None
    if PS:
        kc0, tbl = _paginate(kc0, PS, 3)
        vc0, _ = _paginate(vc0, PS, 3)
    qkv = torch.randn(1, 3 * H * D, **bf)
    cos, sin = rope_tables(rot, L, 10000.0, dev)
    slots = torch.tensor([1], device=dev, dtype=torch.int32)
    pos = torch.tensor([L0 - 1], device=dev, dtype=torch.int32)
    kv_lens = pos + 1
    gx, gw, gb = torch.randn(1, 4096, **bf), torch.randn(16384, 4096, **bf) * 0.02, torch.randn(16384, **bf)
    ws = torch.zeros(max(dops.decode_ws_floats(1, H, H, D, L), 1), device=dev, dtype=torch.float32)
    res = []
    for desc in (False, True):
        kc, vc, out, gy = kc0.clone(), vc0.clone(), torch.empty(1, H * D, **bf), torch.empty(1, 16384, **bf)
        c, s_, t, by = cos, sin, tbl, 0
        if desc:
            c, s_ = cos[L0 - 1:L0].contiguous(), sin[L0 - 1:L0].contiguous()
            by = 1
            if tbl is not None:
                t, by = tbl[1:2].contiguous(), 3
        assert dops.decode_prep_attention_gemv(qkv.clone(), H, H, D, rot, True, c, s_, pos, slots, kc, vc, kv_lens,
                                               L, D ** -0.5, None, out, ws, t, 0, gx, gw, gb, gy, 1, by)
        torch.cuda.synchronize()
        res.append((out, gy, kc, vc))
    (o0, y0, k0, v0), (o1, y1, k1, v1) = res
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert torch.equal(o0, o1)
    assert torch.equal(y0, y1)


def test_engine_fused_b1_step_descriptors_bit_identical(monkeypatch):
    """The fused batch-1 layer with the per-step RoPE / page-row descriptors computes exactly the
    tokens and log-probs of the device-side table lookups."""
    from kubernetes_cloud_amd.engine import runner as runner_mod
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    cfg = dict(PRESETS_HF["gpt-j-6b"])
    cfg.update(n_embd=1024, n_layer=3, n_head=4, rotary_dim=64, n_positions=512)
    m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)
    p = [int(x) for x in torch.randint(0, 1000, (40,))]
    sp = SamplingParams(max_new_tokens=12, do_sample=False, logprobs=True)
    outs = []
    for desc in (True, False):
        monkeypatch.setattr(runner_mod, "_STEP_DESC", desc)
        eng = LLMEngine(m, max_slots=2, max_len=256, use_graphs=True)
        assert eng.runner._fused_ok
        r = eng.generate([p], sp)[0]
        outs.append((r.output, r.logprobs))
    assert outs[0] == outs[1]


def test_engine_step_descriptors_batched_bit_identical(monkeypatch):
    """Batched decode (the unfused per-layer path, paged KV) with the per-step RoPE / page-row
    descriptors gives exactly the tokens and log-probs of the device-side table lookups."""
    from kubernetes_cloud_amd.engine import runner as runner_mod
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    cfg = dict(PRESETS_HF["gpt-j-6b"])
    cfg.update(n_embd=1024, n_layer=2, n_head=4, rotary_dim=64, n_positions=512)
    m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)
    ps = [[int(x) for x in torch.randint(0, 1000, (n,))] for n in (40, 70, 23)]
    sp = SamplingParams(max_new_tokens=10, do_sample=False, logprobs=True)
    outs = []
    for desc in (True, False):
        monkeypatch.setattr(runner_mod, "_STEP_DESC", desc)
        eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True)
        outs.append([(r.output, r.logprobs) for r in eng.generate(ps, sp)])
    assert outs[0] == outs[1]


def test_engine_fused_b1_decode_matches_two_stream():
    """ModelRunner's fused batch-1 GPT-J layer (three launches per layer on one queue) against the
    two-stream form: same greedy tokens where the top-2 logits are not near-tied."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    cfg = dict(PRESETS_HF["gpt-j-6b"])
    cfg.update(n_embd=1024, n_layer=3, n_head=4, rotary_dim=64, n_positions=512)
    m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)
    p = [int(x) for x in torch.randint(0, 1000, (40,))]
    sp = SamplingParams(max_new_tokens=16, do_sample=False)
    outs = []
    for fused in (True, False):
        eng = LLMEngine(m, max_slots=4, max_len=256, use_graphs=True)
        assert eng.runner._fused_ok
        eng.runner._fused_ok = fused
        outs.append(eng.generate([p], sp)[0].output)
    # random-init logits are flat (near-ties flip between the two roundings), so each arm is checked
    # against a full forward of its own continuation: every token with a clear margin is the argmax
    for out in outs:
        with torch.no_grad():
            lg = m(torch.tensor([p + out], device=dev))[0].float()
        for i, t in enumerate(out):
            row = lg[len(p) - 1 + i]
            top2 = row.topk(2).values
            if float(top2[0] - top2[1]) > 0.1:
                assert int(row.argmax()) == t, i


@pytest.mark.parametrize("act", [1, 2])
def test_decode_linear_gelu_many_rows(act):
    """Decode linears past the skinny kernel's rows (hipBLASLt + the native in-place GELU) match
    an fp32 reference."""
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    torch.manual_seed(0)
    M, K, N = 32, 512, 2048
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=dev).to(torch.bfloat16)
    y = skinny_linear(x, w, b, act)
    ref = F.gelu(x.float() @ w.float().t() + b.float(), approximate="tanh" if act == 1 else "none")
    assert (y.float() - ref).abs().max() < 3e-2


def test_sample_multiworkgroup_distribution_and_mixed_rows():
    """GPT-J vocabulary, bf16: rows with 1 <= top_k <= 64 (or greedy) take the multi-workgroup sampler
    (16 chunk workgroups + a last-arriver merge), the others the register kernel, in one call."""
    torch.manual_seed(7)
    V, B, k, p = 50400, 4096, 12, 0.9
    # distinct (bf16-exact) peaks so the top-k / top-p cuts fall between values, not inside a tie group
    # (the kernels keep a whole tie group at a cut; HF's sort keeps an arbitrary part of it)
    base = torch.randn(V, device=dev) * 0.5
    peaks = torch.randperm(V, device=dev)[:20]
    base[peaks] = 4.0 + 0.25 * torch.arange(20, device=dev, dtype=torch.float32)
    base = base.to(torch.bfloat16).float()
    logits = base[None].expand(B, V).contiguous().to(torch.bfloat16)
    seeds = torch.randint(0, 2**62, (B,), device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ids, lp = dops.sample_logits(logits, **_params(B, 1.0, k, p), seeds=seeds, out_kept=kept)
    keep = dops.keep_mask_reference(base, k, p)
    assert bool(keep[ids].all())
    assert int(kept.min()) == int(kept.max()) == int(keep.sum())
    probs = torch.where(keep, base, torch.full_like(base, -float("inf"))).softmax(-1)
    freq = torch.bincount(ids, minlength=V).float() / B
    assert (freq - probs).abs().max() < 0.03
    assert torch.allclose(lp, torch.log_softmax(base, -1)[ids], atol=1e-3)
    # mixed batch: greedy / top-k (multi-workgroup) and top-p only / top-k 100 (register kernel)
    rows = [(0.0, 0, 1.0), (1.0, 50, 0.95), (1.0, 0, 0.9), (0.8, 100, 1.0), (1.0, 10, 1.0), (1.2, 64, 0.5)]
    Bm = len(rows)
    lg = (torch.randn(Bm, V, device=dev) * 3).to(torch.bfloat16)
    t = torch.tensor([r[0] for r in rows], device=dev)
    kk = torch.tensor([r[1] for r in rows], device=dev, dtype=torch.int32)
    pp = torch.tensor([r[2] for r in rows], device=dev)
    out_kept = torch.empty(Bm, dtype=torch.int32, device=dev)
    ids = torch.full((Bm,), -7, dtype=torch.int64, device=dev)
    dops.sample_logits(lg, temperature=t, top_k=kk, top_p=pp, rep_penalty=torch.ones(Bm, device=dev),
                       seeds=torch.arange(Bm, device=dev), out_ids=ids, out_kept=out_kept)
    assert int(ids[0]) == int(lg[0].float().argmax())
    for b, (tb, kb, pb) in enumerate(rows):
        if tb <= 0:
            continue
        x = lg[b].float() / tb
        keep = dops.keep_mask_reference(x, kb, pb)
        tie_incl = x >= x[keep].min()  # the kernels keep whole tie groups at a cut
        assert bool(tie_incl[ids[b]]), (b, rows[b])
        assert int(keep.sum()) <= int(out_kept[b]) <= int(tie_incl.sum()) + 1, (b, rows[b])


@pytest.mark.parametrize("V", [50400, 250880])
@pytest.mark.parametrize("peaked", [True, False])
def test_sample_multiworkgroup_top_p_only(V, peaked):
    """Top-p-only rows (top_k off) on the multi-workgroup sampler: a peaked row's nucleus lies inside the
    chunk candidate lists and the merge samples it (kept set = the HF top-p mask, draw frequencies =
    the renormalised nucleus); a flat row's nucleus does not (its candidates hold < p of the mass), the
    merge marks the row and the one-workgroup kernel launched after it samples it -- same kept set."""
    torch.manual_seed(11)
    B, p = 2048, 0.9
    base = torch.randn(V, device=dev) * (0.5 if peaked else 0.05)
    if peaked:
        peaks = torch.randperm(V, device=dev)[:24]
        base[peaks] = 10.0 + 0.25 * torch.arange(24, device=dev, dtype=torch.float32)
    base = base.to(torch.bfloat16).float()
    logits = base[None].expand(B, V).contiguous().to(torch.bfloat16)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ids, lp = dops.sample_logits(logits, **_params(B, 1.0, 0, p), seeds=torch.randint(0, 2**62, (B,), device=dev),
                                 out_kept=kept)
    keep = dops.keep_mask_reference(base, 0, p)
    tie_incl = base >= base[keep].min()
    assert bool(tie_incl[ids].all())
    assert int(keep.sum()) <= int(kept.min()) and int(kept.max()) <= int(tie_incl.sum())
    assert torch.allclose(lp, torch.log_softmax(base, -1)[ids], atol=1e-3)
    if peaked:  # a few hundred kept tokens at most: the frequencies are testable
        probs = torch.where(keep, base, torch.full_like(base, -float("inf"))).softmax(-1)
        freq = torch.bincount(ids, minlength=V).float() / B
        assert (freq - probs).abs().max() < 0.04


def test_sample_multiworkgroup_wide_ties_take_the_block_path():
    """Tie groups that leave more than 64 candidates after the top-k cut (or more than 256 after the
    chunk cuts) miss the single-wave merge and take the block merge: same selection rules -- the
    whole tie group at the cut is kept, the draw is uniform over it."""
    torch.manual_seed(9)
    V, B = 50400, 2048
    base = torch.randn(V, device=dev) * 0.5
    top = torch.randperm(V, device=dev)[:300]
    base[top] = 5.0  # 300 tied maxima: top-k 20 keeps all 300
    logits = base.to(torch.bfloat16)[None].expand(B, V).contiguous()
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ids, _ = dops.sample_logits(logits, **_params(B, 1.0, 20, 1.0), seeds=torch.randint(0, 2**62, (B,), device=dev),
                                out_kept=kept)
    assert int(kept.min()) == int(kept.max()) == 300
    assert bool((base[ids] == 5.0).all())
    freq = torch.bincount(ids, minlength=V)[top].float()
    assert (freq / B - 1 / 300).abs().max() < 0.01


@pytest.mark.parametrize("B", [1, 3])
def test_engine_lookahead_across_kv_buckets_matches_unpipelined(B):
    """The one-step lookahead launches step t+1 before the host reads step t. When t+1 lands in a
    different kv-length bucket (max_kv crosses 256 -> 257, its own graph and packed inputs), the two
    in-flight steps must still land their sampled ids in different pinned buffers: the pipelined run
    equals the unpipelined one token for token (the landing buffer flips per batch bucket)."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = _gpu_model("gpt-j-6b")
    g = torch.Generator().manual_seed(3)
    # prompts end just below the 256 bucket edge, so the decode crosses it a few tokens in
    prompts = [[int(x) for x in torch.randint(0, 1000, (n,), generator=g)] for n in (250, 245, 200)[:B]]
    sp = SamplingParams(max_new_tokens=24, do_sample=False, logprobs=True)
    outs = []
    for pipe in (False, True):
        eng = LLMEngine(m, max_slots=4, max_len=512, use_graphs=True, pipeline=pipe)
        assert eng.pipeline == pipe
        outs.append([(r.output, r.logprobs) for r in eng.generate(prompts, sp)])
    assert outs[0] == outs[1]


def _small_lm(preset, **over):
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    small = {"gpt-neox-20b": dict(hidden_size=768, num_hidden_layers=3, num_attention_heads=8,
                                  intermediate_size=3072, max_position_embeddings=512),
             "pythia-2.8b": dict(hidden_size=640, num_hidden_layers=3, num_attention_heads=8,
                                 intermediate_size=2560, max_position_embeddings=512),
             "bloom-560m": dict(hidden_size=512, n_layer=3, n_head=4),
             "gpt2": dict(n_embd=512, n_layer=3, n_head=8, n_positions=512)}[preset]
    cfg = dict(PRESETS_HF[preset])
    cfg.update(small, **over)
    return build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)


def _check_against_forward(m, prompt, out, margin=0.1):
    """Every generated token with a clear top-2 margin is the argmax of a full forward (random-init
    logits are flat: near-ties flip between two bf16 roundings of the same math)."""
    with torch.no_grad():
        lg = m(torch.tensor([prompt + out], device=dev))[0].float()
    for i, t in enumerate(out):
        row = lg[len(prompt) - 1 + i]
        top2 = row.topk(2).values
        if float(top2[0] - top2[1]) > margin:
            assert int(row.argmax()) == t, i


@pytest.mark.parametrize("preset,kind", [("gpt-neox-20b", "neox"), ("pythia-2.8b", "neox"),
                                         ("bloom-560m", "seq"), ("gpt2", "seq")])
def test_engine_fused_b1_layer_kinds(preset, kind):
    """The batch-1 fused decode layer for GPT-NeoX (parallel residual, ln_1 and ln_2 of one stream from
    one tail: head_dim 96 / 80, rotate-half RoPE on 25 % of it) and for sequential-residual models
    (BLOOM: ALiBi + embedding LayerNorm; GPT-2: learned positions): greedy tokens of the fused and
    the per-projection paths each match a full forward of their own continuation, with HIP graphs."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    m = _small_lm(preset)
    g = torch.Generator().manual_seed(5)
    p = [int(x) for x in torch.randint(0, 1000, (70,), generator=g)]
    sp = SamplingParams(max_new_tokens=16, do_sample=False)
    outs = []
    for fused in (True, False):
        eng = LLMEngine(m, max_slots=2, max_len=256, use_graphs=True)
        assert eng.runner._fused_ok and eng.runner._layer_kind == kind
        eng.runner._fused_ok = fused
        outs.append(eng.generate([p], sp)[0].output)
    for out in outs:
        _check_against_forward(m, p, out)
    # sampled decode through the fused graph is reproducible
    eng = LLMEngine(m, max_slots=2, max_len=256, use_graphs=True)
    sp2 = SamplingParams(max_new_tokens=12, temperature=0.8, top_k=10, seed=3)
    assert eng.generate([p], sp2)[0].output == eng.generate([p], sp2)[0].output


def test_engine_bloom_tp_emulated_rank_fused():
    """Rank 0 of a TP=4 BLOOM layout on one GPU (parallel/tp_emulation.py): the fused sequential layer
    runs on the shard shapes (row-parallel out-projection / fc_out with their replicated biases in the
    LayerNorm tail, vocab-parallel head tiled to the full vocabulary); its tokens match the model's own
    full forward through the same stand-in collectives."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=1024, n_layer=3, n_head=16, vocab_size=4096)
    m = emulated_rank_model(LMConfig.from_hf(cfg), 4, 0, device=dev)
    assert m.h[0].attn.qkv.weight.shape == (3 * 4 * 64, 1024) and m.lm_head.local_weight().shape[0] == 1024
    g = torch.Generator().manual_seed(9)
    p = [int(x) for x in torch.randint(0, 4096, (50,), generator=g)]
    sp = SamplingParams(max_new_tokens=12, do_sample=False)
    eng = LLMEngine(m, max_slots=2, max_len=256, use_graphs=True)
    assert eng.runner._fused_ok and eng.runner._layer_kind == "seq"
    out = eng.generate([p], sp)[0].output
    _check_against_forward(m, p, out)
    assert m.h[0].attn.out.group.allreduce_calls > 0




@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
@pytest.mark.parametrize("B", [3, 20])
def test_engine_batched_mfma_layer(preset, B):
    """The batch 2..64 matrix-core decode layer (runner._layers_decode_batched: LayerNorm on load from the
    previous tail's row statistics, [QKV | fc_in] / K-concatenated out-proj + fc_out launches for the
    parallel-residual kinds, ALiBi + embedding LayerNorm for BLOOM, learned positions and an odd
    vocabulary for GPT-2), HIP graphs on: every row's greedy tokens match a full forward of its own
    continuation, and so do the per-projection path's."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    over = {"gpt-j-6b": dict(n_embd=1024, n_layer=3, n_head=4, rotary_dim=64, n_positions=512)}.get(preset)
    if over:
        from kubernetes_cloud_amd.models.causal_lm import build_model
        from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
        cfg = dict(PRESETS_HF[preset])
        cfg.update(over)
        m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.bfloat16, seed=0)
    else:
        m = _small_lm(preset)
    g = torch.Generator().manual_seed(B)
    prompts = [[int(x) for x in torch.randint(0, 1000, (int(n),), generator=g)]
               for n in torch.randint(8, 90, (B,), generator=g)]
    sp = SamplingParams(max_new_tokens=10, do_sample=False)
    for batched in (True, False):
        eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True)
        assert eng.runner._batched_ok
        eng.runner._batched_ok = batched
        eng.runner._batched_max_b = 64  # (the layer at every bucket, whatever the per-kind dispatch cap)
        outs = [r.output for r in eng.generate(prompts, sp)]
        assert (eng.runner.batched_steps > 0) == batched
        for p, o in zip(prompts, outs):
            _check_against_forward(m, p, o)


@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m"])
def test_engine_fp16_native_decode(preset, monkeypatch):
    """fp16 serving (the precision of BASELINE config 4's FasterTransformer /
    DS-Inference rows) runs the native decode step -- the fused GEMV layer at batch 1, the matrix-core
    layer at batch > 1, the fp16 attention / LayerNorm-row / embedding-head instantiations and the sampler
    reading fp16 logits -- with HIP graphs: the PyTorch fallbacks of the decode attention and the sampler
    are made to fail, greedy tokens match a full fp16 forward, and seeded sampling is reproducible."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    from kubernetes_cloud_amd.ops import decode as dmod
    small = {"gpt-j-6b": dict(n_embd=1024, n_layer=3, n_head=4, rotary_dim=64, n_positions=512),
             "gpt-neox-20b": dict(hidden_size=768, num_hidden_layers=3, num_attention_heads=8,
                                  intermediate_size=3072, max_position_embeddings=512),
             "bloom-560m": dict(hidden_size=512, n_layer=3, n_head=4)}[preset]
    cfg = dict(PRESETS_HF[preset])
    cfg.update(small)
    m = build_model(LMConfig.from_hf(cfg), device=dev, dtype=torch.float16, seed=0)

    def boom(*a, **k):
        raise AssertionError("fp16 decode fell back to PyTorch")
    monkeypatch.setattr(dmod, "decode_attention_reference", boom)
    monkeypatch.setattr(dmod, "sample_logits_reference", boom)
    from kubernetes_cloud_amd.ops import gemv as gmod
    monkeypatch.setattr(gmod, "_act_ref", boom)  # the per-projection path's GELU: fp16 kernel, not eager
    g = torch.Generator().manual_seed(3)
    for B in (1, 5, 20):  # 20: above the GPT-J / BLOOM matrix-core cap -> the per-projection path in fp16
        prompts = [[int(x) for x in torch.randint(0, 1000, (30 + 7 * (i % 5),), generator=g)] for i in range(B)]
        eng = LLMEngine(m, max_slots=B, max_len=256, use_graphs=True)
        assert eng.runner._batched_ok
        outs = [r.output for r in eng.generate(prompts, SamplingParams(max_new_tokens=12, do_sample=False))]
        if B == 1:
            assert eng.runner.fused_steps > 0
        elif B <= eng.runner._batched_max_b:
            assert eng.runner.batched_steps > 0
        else:
            assert eng.runner.batched_steps == 0
        for p, o in zip(prompts, outs):
            _check_against_forward(m, p, o)
        sp = SamplingParams(max_new_tokens=8, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=17)
        a = [r.output for r in eng.generate(prompts, sp)]
        b = [r.output for r in eng.generate(prompts, sp)]
        assert a == b and all(len(x) == 8 for x in a)


def test_engine_batched_mfma_bloom_tp_emulated_rank():
    """Rank 0 of a TP=4 BLOOM layout (parallel/tp_emulation.py) at batch 6 through the matrix-core layer:
    shard shapes, vocab-parallel head gathered by the stand-in group."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=1024, n_layer=3, n_head=16, vocab_size=4096)
    m = emulated_rank_model(LMConfig.from_hf(cfg), 4, 0, device=dev)
    g = torch.Generator().manual_seed(11)
    prompts = [[int(x) for x in torch.randint(0, 4096, (40 + 3 * i,), generator=g)] for i in range(6)]
    eng = LLMEngine(m, max_slots=8, max_len=256, use_graphs=True)
    outs = [r.output for r in eng.generate(prompts, SamplingParams(max_new_tokens=10, do_sample=False))]
    assert eng.runner.batched_steps > 0
    for p, o in zip(prompts, outs):
        _check_against_forward(m, p, o)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_engine_emulated_rank_runs_real_tp_tails(dtype):
    """with a rank-local custom all-reduce registered for the emulated group, rank 0 of a
    TP=4 BLOOM layout closes every row-parallel projection with the deployment's fused all-reduce tails
    (kca_ar_res_ln at batch 1, kca_ar_res_stats at batch > 1; fp16 -- DS-Inference's precision -- their
    _f16 twins) -- the kernels bench/bloom_tp_bench.py then measures -- and still
    matches the model's own forward through the same stand-in collectives."""
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
    from kubernetes_cloud_amd.parallel.custom_ar import register
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=1024, n_layer=3, n_head=16, vocab_size=4096)
    m = emulated_rank_model(LMConfig.from_hf(cfg), 4, 0, device=dev, dtype=dtype)
    ar = register(m.h[0].attn.out.group)
    assert ar is not None and ar.world == 1
    g = torch.Generator().manual_seed(13)
    prompts = [[int(x) for x in torch.randint(0, 4096, (30 + 7 * i,), generator=g)] for i in range(6)]
    eng = LLMEngine(m, max_slots=8, max_len=256, use_graphs=True)
    assert eng.runner._tp_ar is ar and eng.runner._batched_ok
    sp = SamplingParams(max_new_tokens=10, do_sample=False)
    outs = [eng.generate([prompts[0]], sp)[0].output] + [r.output for r in eng.generate(prompts, sp)]
    assert ar.res_ln_calls > 0 and ar.res_stats_calls > 0 and ar.error() == 0
    assert eng.runner.step_launches  # launches per step recorded for the bench
    for p, o in zip([prompts[0]] + prompts, outs):
        _check_against_forward(m, p, o)
