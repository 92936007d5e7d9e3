"""Speculative decoding on the CPU: the multi-token attention reference against the one-token reference
row by row, the n-gram proposer, and the engine's draft-and-verify loop on tiny fp32 models against the
same engine without speculation -- token for token, with the accepted / drafted counts a scripted
proposer implies."""
import pytest
import torch

from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.engine.runner import KVCacheFull, ModelRunner
from kubernetes_cloud_amd.engine.spec import NgramProposer
from kubernetes_cloud_amd.models.causal_lm import build_model
from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
from kubernetes_cloud_amd.ops import decode as dops
from kubernetes_cloud_amd.ops import spec

from .test_kv8_cpu import SMALL, _paginate

TINY = dict(SMALL)
TINY["gpt-neox-20b"] = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
                            max_position_embeddings=64)
VOCAB = 97


def tiny(preset):
    cfg = dict(PRESETS_HF[preset])
    cfg.update(TINY[preset])
    cfg.update(vocab_size=VOCAB)
    return build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)


# ------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("alibi,window", [(False, 0), (True, 0), (True, 40), (False, 40)])
@pytest.mark.parametrize("fp64", [False, True])
def test_reference_is_the_one_token_reference_row_by_row(PS, alibi, window, fp64):
    g = torch.Generator().manual_seed(PS + window + alibi)
    S, Hkv, G, L, D, T = 3, 2, 2, 64, 16, 4
    H = Hkv * G
    k = torch.randn(S, Hkv, L, D, generator=g)
    v = torch.randn(S, Hkv, L, D, generator=g)
    tbl = None
    if PS:
        perm = torch.randperm(S * L // PS, generator=g)
        k, v = _paginate(k, PS, perm), _paginate(v, PS, perm)
        tbl = perm.view(S, L // PS).to(torch.int32)
    slots = torch.tensor([2, 0, 1], dtype=torch.int32)
    kv_lens = torch.tensor([61, 18, 3], dtype=torch.int32)  # the third: an empty cache before the step
    n_tok = torch.tensor([4, 2, 3], dtype=torch.int32)
    q = torch.randn(S * T, H * D, generator=g)
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625]) if alibi else None
    out = spec.spec_attention_reference(q, k, v, slots, kv_lens, n_tok, T, H, 0.25, slopes, block_table=tbl,
                                        window=window, fp64=fp64)
    via_op = spec.spec_attention(q, k, v, slots, kv_lens, n_tok, T, H, 64, 0.25, slopes, block_table=tbl,
                                 window=window)
    n_rows = 0
    for b in range(S):
        for t in range(T):
            r = b * T + t
            if t >= int(n_tok[b]):
                assert not out[r].any() and not via_op[r].any()
                continue
            one = dops.decode_attention_reference(
                q[r:r + 1], k, v, slots[b:b + 1], kv_lens[b:b + 1] - n_tok[b] + t + 1, H, 0.25, slopes,
                block_table=tbl, window=window)
            if fp64:
                torch.testing.assert_close(out[r:r + 1], one, rtol=1e-5, atol=1e-6)
            else:
                assert torch.equal(out[r:r + 1], one)
                assert torch.equal(via_op[r:r + 1], one)
            n_rows += 1
    assert n_rows == 9


@pytest.mark.parametrize("PS", [0, 16])
@pytest.mark.parametrize("rot,inter", [(0, False), (8, True), (16, False)])
def test_prep_reference_is_decode_prep_row_by_row(PS, rot, inter):
    from kubernetes_cloud_amd.ops.rope import rope_tables
    g = torch.Generator().manual_seed(rot + PS)
    S, H, Hkv, L, D, B, T = 4, 4, 2, 32, 16, 3, 4
    cos, sin = rope_tables(rot, L, 10000.0, "cpu") if rot else (None, None)
    base = torch.tensor([13, 0, 27], dtype=torch.int32)
    n_tok = torch.tensor([4, 1, 3], dtype=torch.int32)
    slots = torch.tensor([3, 1, 0], dtype=torch.int32)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, generator=g)
    shape = (S * L // PS + 1, Hkv, PS, D) if PS else (S, Hkv, L, D)
    tbl = torch.randperm(S * L // PS, generator=g).to(torch.int32).view(S, L // PS) if PS else None
    ka, va = torch.full(shape, float("nan")), torch.full(shape, float("nan"))
    kb, vb = ka.clone(), va.clone()
    a, b_ = qkv.clone(), qkv.clone()
    spec.spec_prep(a, H, Hkv, D, rot, inter, cos, sin, base, n_tok, slots, T, ka, va, tbl)
    rows = [(b, t) for b in range(B) for t in range(int(n_tok[b]))]
    idx = torch.tensor([b * T + t for b, t in rows])
    sub = b_[idx].contiguous()
    dops.decode_prep(sub, H, Hkv, D, rot, inter, cos, sin,
                     torch.tensor([int(base[b]) + t for b, t in rows], dtype=torch.int32),
                     torch.tensor([int(slots[b]) for b, _ in rows], dtype=torch.int32), kb, vb, tbl)
    b_[idx] = sub
    assert torch.equal(a, b_)  # padding rows untouched, real rows rotated alike
    assert torch.equal(ka.nan_to_num(7.0), kb.nan_to_num(7.0)) and torch.equal(va.nan_to_num(7.0), vb.nan_to_num(7.0))
    assert int((~torch.isnan(ka[..., 0])).sum()) == len(rows) * Hkv  # nothing else written


def test_supported():
    assert spec.supported(256, 16, 16, 8) and spec.supported(96, 64, 64, 2) and spec.supported(64, 8, 4, 4)
    assert spec.supported(128, 8, 2, 2)
    assert spec.supported(72, 4, 4, 4) and not spec.supported(72, 6, 2, 2) and not spec.supported(76, 4, 4, 4) and not spec.supported(64, 8, 4, 8) and not spec.supported(64, 8, 2, 4)
    assert not spec.supported(64, 4, 4, 3) and not spec.supported(64, 4, 4, 1) and not spec.supported(264, 4, 4, 2)


# -------------------------------------------------------------------------------------- proposer
def test_ngram_longest_n_first_and_latest_match():
    p = NgramProposer(max_ngram=3, min_ngram=1)
    #        0  1  2  3  4  5  6  7  8  9 10 11 12 13
    toks = [1, 2, 3, 9, 5, 2, 3, 8, 1, 2, 3, 7, 2, 3]
    # the 3-gram (7, 2, 3) has no earlier occurrence; the 2-gram (2, 3) occurs at 1, 5 and 9: the latest wins
    assert p.propose(toks, 3) == [7, 2, 3]
    assert p.propose(toks, 1) == [7]
    # a 3-gram match is preferred to a later 2-gram match
    toks = [4, 5, 6, 10, 11, 5, 6, 12, 13, 4, 5, 6]
    assert p.propose(toks, 2) == [10, 11]
    assert NgramProposer(max_ngram=2).propose(toks, 2) == [12, 13]
    # n = 1 as the last resort
    assert p.propose([3, 1, 4, 1], 5) == [4, 1]


def test_ngram_window_no_match_and_k():
    toks = [1, 2, 3, 4] + list(range(10, 30)) + [1, 2]
    assert NgramProposer(window=1024).propose(toks, 2) == [3, 4]
    assert NgramProposer(window=20).propose(toks, 2) == []  # the earlier (1, 2) lies outside the window
    assert NgramProposer().propose([1, 2, 3, 4, 5], 4) == []
    assert NgramProposer().propose([7], 4) == [] and NgramProposer().propose([], 4) == []
    rep = [1, 2, 3] * 6
    for k in (0, 1, 2, 3):
        assert len(NgramProposer().propose(rep, k)) == k
    assert NgramProposer().propose(rep, 5) == [1, 2, 3]  # the latest match: three tokens follow it
    assert NgramProposer().propose(rep + [1], 5) == [2, 3, 1]
    assert NgramProposer().propose([5, 5], 4) == [5]  # never more than what followed the match
    with pytest.raises(ValueError):
        NgramProposer(max_ngram=1, min_ngram=2)


# ---------------------------------------------------------------------------------------- engine
class Scripted:
    """Drafts a known continuation (``scripts[prompt]``: the expected output) while the request's output
    is still a prefix of it, with a wrong token planted at the output indices in ``wrong`` and at most
    ``cap`` tokens per call."""

    def __init__(self, scripts, wrong=(), cap=None):
        self.scripts = {tuple(p): list(o) for p, o in scripts.items()}
        self.wrong, self.cap, self.calls = set(wrong), cap, 0

    def draft(self, prompt, out, k):
        full = self.scripts[tuple(prompt)]
        i = len(out)
        if list(out) != full[:i]:
            return []
        k = k if self.cap is None else min(k, self.cap)
        return [(t + 1) % VOCAB if j in self.wrong else t for j, t in enumerate(full[i:i + k], start=i)]

    def propose(self, tokens, k):
        self.calls += 1
        for p in self.scripts:
            if tuple(tokens[:len(p)]) == p and len(tokens) > len(p):
                return self.draft(p, tokens[len(p):], k)
        raise AssertionError("unknown prompt")


def implied(script: Scripted, prompt, out, T, max_new):
    """(verify steps, drafted, accepted) a single request's run implies: ``out`` is its final output."""
    i, steps, drafted, accepted = 1, 0, 0, 0  # the first token comes from prefill
    while i < len(out):
        d = script.draft(prompt, out[:i], min(T - 1, max_new - i - 1))
        if not d:
            i += 1
            continue
        steps += 1
        drafted += len(d)
        e = 1
        while e <= len(d) and d[e - 1] == out[i + e - 1] and i + e < len(out):
            e += 1
        accepted += e - 1
        i += e
    return steps, drafted, accepted


PROMPT = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]
GREEDY = dict(do_sample=False)
SAMPLED = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.95, seed=11)


def run(m, prompts, sp, **kw):
    eng = LLMEngine(m, max_slots=4, max_len=48, **kw)
    reqs = eng.generate(prompts, sp)
    return [r.output for r in reqs], [r.finish_reason for r in reqs], eng


CASES = {
    # name: (T, wrong offsets, cap, max_new, extra sampling parameters as a function of the free-running output)
    "all accepted": (4, (), None, 14, None),
    "first draft wrong": (4, (1, 5, 9), None, 14, None),
    "middle draft wrong": (4, (2, 6, 11), None, 14, None),
    "draft shorter than T-1": (4, (), 1, 14, None),
    "T=8, clipped by max_new_tokens": (8, (), None, 6, None),
    "T=2": (2, (3,), None, 9, None),
    "eos inside an accepted run": (4, (), None, 14, lambda o: dict(eos_token_id=o[5])),
    "min_new_tokens bans an eos draft": (4, (), None, 14, lambda o: dict(eos_token_id=o[2], min_new_tokens=6)),
    "stop sequence completed mid-run": (4, (), None, 14, lambda o: dict(stop_sequences=[[o[5], o[6]]])),
}


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("preset,page", [("gpt-j-6b", 16), ("gpt-neox-20b", 0), ("bloom-560m", 16), ("gpt2", 0)])
def test_engine_equals_the_baseline(preset, page, case, mode):
    T, wrong, cap, max_new, extra = CASES[case]
    m = tiny(preset)
    base = dict(GREEDY if mode == "greedy" else SAMPLED)
    free, _, _ = run(m, [PROMPT], SamplingParams(max_new_tokens=max_new, **base), page_size=page)
    kw = extra(free[0]) if extra else {}
    sp = SamplingParams(max_new_tokens=max_new, **base, **kw)
    want, why, eng0 = run(m, [PROMPT], sp, page_size=page)
    assert eng0.stats["spec_steps"] == 0
    # the script drafts the free-running continuation: past an eos / a stop sequence, and an eos that
    # min_new_tokens bans
    script = Scripted({tuple(PROMPT): free[0]}, wrong, cap)
    got, why2, eng = run(m, [PROMPT], sp, page_size=page, spec_tokens=T, proposer=script)
    assert got == want and why2 == why
    # the tied-embedding tiny models (bloom, gpt2) repeat one token under greedy decoding: an eos or a
    # stop sequence taken from that output ends the request at its first token, before any verify step
    # (the sampled runs of the same models, and both modes of the other two, do reach it mid-run)
    degenerate = len(set(free[0])) == 1
    if extra and not degenerate:
        assert len(want[0]) < max_new or "min_new" in case  # the finish really falls inside the run
    steps, drafted, accepted = implied(script, PROMPT, want[0], T, max_new)
    st = eng.stats
    print(f"{preset} {case} {mode}: {len(want[0])} tokens, {st['spec_steps']} verify steps, "
          f"{st['spec_accepted']} of {st['spec_drafted']} drafts accepted")
    assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == (steps, drafted, accepted)
    assert (steps > 0 or (degenerate and extra is not None)) and st["decode_tokens"] == len(want[0]) - 1
    assert eng.runner.spec_steps == steps
    if case == "all accepted":
        assert accepted == drafted > 0
    if "wrong" in case:
        assert 0 < accepted < drafted


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_engine_batch_with_riders(mode):
    """Four requests in one batch: two with drafts, one with a repetition penalty and one with a multi-token
    bad word (no drafts: n = 1 rows of the same verify step); logprobs too."""
    m = tiny("gpt-j-6b")
    base = dict(GREEDY if mode == "greedy" else SAMPLED)
    prompts = [PROMPT, PROMPT[2:] + [7, 7], [8, 2, 8, 1, 8, 2, 8], [6, 6, 2, 6, 4, 6]]
    free, _, _ = run(m, prompts, SamplingParams(max_new_tokens=10, **base), page_size=16)
    sps = [SamplingParams(max_new_tokens=10, logprobs=True, **base),
           SamplingParams(max_new_tokens=8, bad_words_ids=[[free[1][3]]], **base),
           SamplingParams(max_new_tokens=10, repetition_penalty=1.3, **base),
           SamplingParams(max_new_tokens=10, bad_words_ids=[[free[3][2], free[3][3]]], **base)]
    eng0 = LLMEngine(m, max_slots=4, max_len=48, page_size=16)
    want = eng0.generate(prompts, sps)
    assert want[3].output[3] != free[3][3]  # the bad word did bite
    script = Scripted({tuple(p): r.output for p, r in zip(prompts, want)}, wrong=(4,))
    eng = LLMEngine(m, max_slots=4, max_len=48, page_size=16, spec_tokens=4, proposer=script)
    log, real = [], eng._drafts

    def spy(r):
        d = real(r)
        log.append((r.rid, len(d)))
        return d

    eng._drafts = spy
    got = eng.generate(prompts, sps)
    assert [r.output for r in got] == [r.output for r in want]
    torch.testing.assert_close(torch.tensor(got[0].logprobs), torch.tensor(want[0].logprobs), rtol=1e-4, atol=1e-5)
    assert eng.stats["spec_steps"] > 0 and eng.stats["spec_accepted"] > 0
    assert eng.stats["decode_tokens"] == sum(len(r.output) - 1 for r in got)
    assert {rid for rid, _ in log} == {0, 1, 2, 3}
    assert all(n == 0 for rid, n in log if rid in (2, 3))  # the riders: one token per step
    assert any(n == 3 for rid, n in log if rid == 0)


def test_engine_ngram_on_a_repeating_prompt():
    m = tiny("gpt2")
    prompt = [5, 6, 7, 8] * 5
    sp = SamplingParams(max_new_tokens=12, do_sample=False)
    want, _, _ = run(m, [prompt], sp)
    got, _, eng = run(m, [prompt], sp, spec_tokens=4)
    assert isinstance(eng.proposer, NgramProposer)
    assert got == want and eng.stats["spec_steps"] > 0 and eng.stats["spec_drafted"] > 0
    sp = SamplingParams(max_new_tokens=12, **SAMPLED)
    assert run(m, [prompt], sp, spec_tokens=8)[0] == run(m, [prompt], sp)[0]


def test_engine_exact_page_budget():
    """kv_pages = the admitted worst case: drafts never reach past prompt + max_new_tokens, so the run
    ends without KVCacheFull and every page comes back."""
    m = tiny("gpt-j-6b")
    max_new = 48 - len(PROMPT)  # up to max_len too
    sp = SamplingParams(max_new_tokens=max_new, do_sample=False)
    want, _, _ = run(m, [PROMPT], sp, page_size=16)
    eng = LLMEngine(m, max_slots=2, max_len=48, page_size=16, kv_pages=3, spec_tokens=8,
                    proposer=Scripted({tuple(PROMPT): want[0]}))
    start = eng.runner.cache.free_count()
    assert start == 3 == eng.runner.cache.pages_for(len(PROMPT) + max_new)
    try:
        got = eng.generate([PROMPT], sp)
    except KVCacheFull as e:  # pragma: no cover
        pytest.fail(str(e))
    assert got[0].output == want[0] and len(want[0]) == max_new
    assert eng.runner.cache.free_count() == start
    assert eng.stats["spec_accepted"] == eng.stats["spec_drafted"] > 0


# --------------------------------------------------------------------------------------- options
def test_off_by_default_and_option_values(monkeypatch):
    m = tiny("gpt-j-6b")
    monkeypatch.delenv("KCA_DECODE_SPEC", raising=False)

    def boom(self, rows):
        raise AssertionError("verify called with speculation off")

    monkeypatch.setattr(ModelRunner, "verify", boom)
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.spec_tokens == 0 and eng.runner.spec_tokens == 0 and eng.proposer is None
    eng.generate([[1, 2, 3, 1, 2, 3, 1, 2]], SamplingParams(max_new_tokens=6, do_sample=False))
    assert eng.stats["spec_steps"] == 0 and eng.runner.spec_steps == 0
    for off in ("0", "none", "off", ""):
        monkeypatch.setenv("KCA_DECODE_SPEC", off)
        assert LLMEngine(m, max_slots=2, max_len=32).spec_tokens == 0
    monkeypatch.undo()
    monkeypatch.setenv("KCA_DECODE_SPEC", "4")
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.spec_tokens == 4 and eng.runner.spec_tokens == 4 and not eng.pipeline
    eng.generate([[1, 2, 3, 1, 2, 3, 1, 2]], SamplingParams(max_new_tokens=6, do_sample=False))
    assert LLMEngine(m, max_slots=2, max_len=32, spec_tokens=0).spec_tokens == 0  # the keyword wins
    monkeypatch.setenv("KCA_DECODE_SPEC", "3")
    with pytest.raises(ValueError, match="KCA_DECODE_SPEC.*3"):
        LLMEngine(m, max_slots=2, max_len=32)
    monkeypatch.setenv("KCA_DECODE_SPEC", "many")
    with pytest.raises(ValueError, match="KCA_DECODE_SPEC.*many"):
        LLMEngine(m, max_slots=2, max_len=32)
    monkeypatch.delenv("KCA_DECODE_SPEC")
    for T in (2, 4, 8):
        assert ModelRunner(m, max_slots=2, max_len=32, spec_tokens=T).spec_tokens == T
    for bad in (1, 3, 5, 16, -2):
        with pytest.raises(ValueError, match="spec_tokens"):
            ModelRunner(m, max_slots=2, max_len=32, spec_tokens=bad)
    with pytest.raises(ValueError, match="pipeline"):
        LLMEngine(m, max_slots=2, max_len=32, spec_tokens=4, pipeline=True)
    with pytest.raises(ValueError, match="propose"):
        LLMEngine(m, max_slots=2, max_len=32, spec_tokens=4, proposer=object())
    runner = ModelRunner(m, max_slots=2, max_len=32, spec_tokens=2)
    assert LLMEngine(m, runner=runner).spec_tokens == 2
    with pytest.raises(ValueError, match="spec_tokens.*runner"):
        LLMEngine(m, runner=runner, spec_tokens=2)
    with pytest.raises(RuntimeError, match="spec_tokens"):
        ModelRunner(m, max_slots=2, max_len=32).verify_async([])


def test_refusals():
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    m = tiny("gpt-j-6b")
    with pytest.raises(ValueError, match="fp8"):
        LLMEngine(m, max_slots=2, max_len=32, spec_tokens=4, kv_dtype="fp8")
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=64, n_layer=2, n_head=4, vocab_size=96)
    tp = emulated_rank_model(LMConfig.from_hf(cfg), 2, 0, dtype=torch.float32)
    with pytest.raises(ValueError, match="tensor-parallel"):
        LLMEngine(tp, max_slots=2, max_len=32, spec_tokens=4)
    split = tiny("gpt-j-6b")
    split.h[1].to("meta")  # a second device under the last layer: a layer-split placement
    with pytest.raises(ValueError, match="layer-split"):
        LLMEngine(split, max_slots=2, max_len=32, spec_tokens=4)
    cfg = dict(PRESETS_HF["gpt2"])
    cfg.update(n_embd=48, n_layer=1, n_head=4, n_positions=32, vocab_size=50)  # head_dim 12
    odd = build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)
    with pytest.raises(ValueError, match="head_dim 12"):
        LLMEngine(odd, max_slots=2, max_len=32, spec_tokens=4)
    # four query heads per KV head: 4 x 4 queries do not fit the kernel's eight, 4 x 2 do
    r = ModelRunner(m, max_slots=2, max_len=32)
    r.Hkv = 1
    with pytest.raises(ValueError, match="4 query heads per KV head"):
        r._spec_tokens(4)
    assert r._spec_tokens(2) == 2
    # rows outside 1..T tokens, or past max_len
    r = ModelRunner(m, max_slots=2, max_len=32, spec_tokens=2)
    row = dict(pos=3, slot=0, temperature=0.0, top_k=0, top_p=1.0, rep=1.0)
    with pytest.raises(ValueError, match="1..2 tokens"):
        r.verify([dict(row, tokens=[1, 2, 3], seeds=[0, 0, 0], bans=[(), (), ()])])
    with pytest.raises(ValueError, match="max_len"):
        r.verify([dict(row, pos=31, tokens=[1, 2], seeds=[0, 0], bans=[(), ()])])
