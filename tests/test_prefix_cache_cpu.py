"""Prefix caching on the CPU: the paged prefill attention reference against ``ops.attention_reference`` row by
row, the cache's prefix index (chained lookup, the cap, duplicates, refcounts, LRU leaf-first eviction, an
exact page budget) and the engine with ``prefix_cache=True`` on tiny fp32 models against the same engine
without it -- token for token."""
import pytest
import torch

from kubernetes_cloud_amd import ops
from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
from kubernetes_cloud_amd.engine.runner import KVCache, KVCacheFull, ModelRunner
from kubernetes_cloud_amd.models.causal_lm import build_model
from kubernetes_cloud_amd.models.config import PRESETS_HF, LMConfig
from kubernetes_cloud_amd.ops import prefill_paged as pp

from .test_kv8_cpu import _paginate
from .test_spec_cpu import GREEDY, SAMPLED, VOCAB, Scripted, tiny

PS = 16


# ------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("fp64", [False, True])
def test_reference_is_attention_reference_row_by_row(page, alibi, fp64):
    g = torch.Generator().manual_seed(page + alibi)
    S, Hkv, G, L, D, T = 4, 2, 2, 64, 16, 20
    H = Hkv * G
    k, v = torch.randn(S, Hkv, L, D, generator=g), torch.randn(S, Hkv, L, D, generator=g)
    kc, vc, tbl = k, v, None
    if page:
        perm = torch.randperm(S * L // page, generator=g)
        kc, vc = _paginate(k, page, perm), _paginate(v, page, perm)
        tbl = perm.view(S, L // page).to(torch.int32)
    slots = torch.tensor([2, 0, 3], dtype=torch.int32)
    start = torch.tensor([0, 37, 16], dtype=torch.int32)
    lens = torch.tensor([20, 5, 1], dtype=torch.int32)
    q = torch.randn(3, T, H, D, generator=g)
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625]) if alibi else None
    out = pp.prefill_paged_attention_reference(q, kc, vc, slots, start, lens, 0.25, slopes, block_table=tbl,
                                               fp64=fp64)
    via_op = pp.prefill_paged_attention(q, kc, vc, slots, start, lens, 0.25, slopes, block_table=tbl)
    for r in range(3):
        p0, n, s_ = int(start[r]), int(lens[r]), int(slots[r])
        assert not out[r, n:].any() and not via_op[r, n:].any()
        kw = k[s_, :, :p0 + n].transpose(0, 1)[None]
        vw = v[s_, :, :p0 + n].transpose(0, 1)[None]
        one, _ = ops.attention_reference(q[r:r + 1, :n], kw, vw, causal=True, scale=0.25, alibi=slopes)
        torch.testing.assert_close(out[r:r + 1, :n], one, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(via_op[r:r + 1, :n], one, rtol=1e-5, atol=1e-6)
        if not fp64:
            assert torch.equal(via_op[r], out[r])


def test_supported():
    assert pp.supported(256, 16, 16, 0) and pp.supported(96, 64, 64) and pp.supported(64, 8, 2) and pp.supported(72, 4, 4)
    assert not pp.supported(64, 8, 8, 256) and not pp.supported(76, 4, 4) and not pp.supported(264, 4, 4)
    assert not pp.supported(64, 6, 4)


def test_dispatch_keeps_the_gather_loop_where_it_measured_faster():
    """``ModelRunner._paged_prefill``: the kernel wherever it covers the layer, except one bf16 GPU row of
    >= 512 queries behind >= 2048 cached tokens (docs/PERF.md, Round 14)."""
    import types
    at, local = types.SimpleNamespace(window=0), types.SimpleNamespace(window=256)
    gpu = types.SimpleNamespace(D=96, H=64, Hkv=64, dtype=torch.bfloat16, device=torch.device("cuda", 0))
    ask = lambda r, *a: ModelRunner._paged_prefill(r, *a)  # noqa: E731
    assert not ask(gpu, at, 1, 512, [2048]) and not ask(gpu, at, 1, 700, [4096])
    assert ask(gpu, at, 1, 511, [2048]) and ask(gpu, at, 1, 512, [2047]) and ask(gpu, at, 2, 512, [2048, 0])
    assert not ask(gpu, local, 8, 64, [64] * 8)
    gpu.dtype = torch.float16
    assert ask(gpu, at, 1, 512, [2048])
    cpu = types.SimpleNamespace(D=96, H=64, Hkv=64, dtype=torch.bfloat16, device=torch.device("cpu"))
    assert ask(cpu, at, 1, 512, [2048])


# ----------------------------------------------------------------------------------------- index
def _cache(n_pages=12, slots=4, max_len=64):
    c = KVCache(1, slots, 1, max_len, 8, "cpu", torch.float32, page_size=PS, n_pages=n_pages)
    c.enable_prefix_index()
    return c


def _toks(*pages):
    """A token list of full pages: page value p stands for 16 tokens [p, p, ...]."""
    return [p for pg in pages for p in [pg] * PS]


def test_index_chained_lookup_cap_and_duplicates():
    c = _cache()
    start = c.free_count()
    a = _toks(1, 2, 3)
    c.reserve(0, len(a))
    assert c.register(0, a, 3) == 3 and c.register(0, a, 3) == 0
    pages_a = list(c.pages[0])
    # a second prompt sharing 2 of 3 pages matches exactly 2; a page under another parent does not match
    assert c.lookup(_toks(1, 2, 9), 3) == pages_a[:2]
    assert c.lookup(_toks(2, 3), 2) == [] and c.lookup(_toks(9, 2, 3), 3) == []
    assert c.lookup(a + [5], 3) == pages_a and c.lookup(a, 2) == pages_a[:2]  # the caller's cap
    # keys compare by value: one differing token in a page is a miss from there on
    b = list(a)
    b[PS + 3] += 1
    assert c.lookup(b, 3) == pages_a[:1]
    # a duplicate registration keeps the first page, and nothing under the duplicate is registered
    dup = _toks(1, 2, 7)
    c.reserve(1, len(dup))
    assert c.register(1, dup, 3) == 0
    assert c.lookup(dup, 3) == pages_a[:2]
    # an adopted chain continues: the slot registers its own third page under the shared second
    c.release(1)
    c.adopt(1, pages_a[:2])
    assert [c.ref[p] for p in pages_a] == [3, 3, 2]
    c.reserve(1, len(dup))
    assert c.pages[1][:2] == pages_a[:2] and c.register(1, dup, 3) == 1
    assert c.lookup(dup, 3) == c.pages[1]
    # refcounts: slots gone -> the index alone (1 each); index cleared -> zero, every page free again
    c.release(0)
    c.release(1)
    assert sorted(x for x in c.ref if x) == [1, 1, 1, 1] and c.free_count() == start
    assert len(c.free_pages) == start - 4
    c.clear_prefix_index()
    assert not any(c.ref) and len(c.free_pages) == start and c.lookup(a, 3) == []


def test_index_eviction_is_lru_and_leaf_first():
    c = _cache(n_pages=6, max_len=128)
    a, b = _toks(1, 2, 3), _toks(4, 5)
    for slot, t in ((0, a), (1, b)):
        c.reserve(slot, len(t))
        c.register(slot, t, len(t) // PS)
    pa, pb = list(c.pages[0]), list(c.pages[1])
    c.release(0)
    c.release(1)
    assert c.free_count() == 6 and len(c.free_pages) == 1
    held = lambda: set(c._pinfo)  # noqa: E731  (registered pages, read without refreshing anything)
    # uses so far: a registered, then b registered, then a hit on a's first two pages. Least recently used
    # first, the deeper page first among equals: a's third page, b's second, b's first, a's second, a's first
    assert c.lookup(a, 2) == pa[:2]
    c.reserve(2, 2 * PS)  # needs 2, 1 free: one eviction
    assert c.prefix_evictions == 1 and held() == {pa[0], pa[1], pb[0], pb[1]}
    c.reserve(2, 3 * PS)  # b's leaf goes before b's root
    assert c.prefix_evictions == 2 and held() == {pa[0], pa[1], pb[0]}
    c.reserve(2, 4 * PS)
    assert c.prefix_evictions == 3 and held() == {pa[0], pa[1]}
    c.reserve(3, PS)  # a's second page before a's first: same age, deeper
    assert held() == {pa[0]}
    with pytest.raises(KVCacheFull):
        c.reserve(3, 3 * PS)  # one evictable page left, two needed: nothing is evicted for it
    assert c.free_count() == 1 and held() == {pa[0]} and c.prefix_evictions == 4
    # a page in use is never evicted
    c.release(2)
    c.release(3)
    c.adopt(0, c.lookup(a, 1))
    c.reserve(1, 5 * PS)
    with pytest.raises(KVCacheFull):
        c.reserve(2, PS)
    assert c.lookup(a, 1) == pa[:1]


# ---------------------------------------------------------------------------------------- engine
def _prompts(seed=0):
    g = torch.Generator().manual_seed(seed)
    pre = torch.randint(0, VOCAB, (2 * PS,), generator=g).tolist()
    return pre + [5, 6, 7], pre + [9, 1, 2, 3, 4]


def _serve(m, prompts, sps, **kw):
    """Requests one after the other on one engine: (outputs, finish reasons, engine)."""
    eng = LLMEngine(m, max_slots=4, max_len=64, page_size=PS, **kw)
    reqs = [eng.generate([p], sp)[0] for p, sp in zip(prompts, sps)]
    return [r.output for r in reqs], [r.finish_reason for r in reqs], eng


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("preset", ["gpt-j-6b", "gpt-neox-20b", "bloom-560m", "gpt2"])
def test_engine_hit_equals_the_engine_without(preset, mode):
    m = tiny(preset)
    sp = SamplingParams(max_new_tokens=8, **(GREEDY if mode == "greedy" else SAMPLED))
    A, B = _prompts()
    want, why, eng0 = _serve(m, [A, B], [sp, sp])
    got, why2, eng = _serve(m, [A, B], [sp, sp], prefix_cache=True)
    assert got == want and why2 == why
    assert "prefix_hit_tokens" not in eng0.stats and not eng0.runner.prefix_cache
    st = eng.stats
    assert st["prefix_lookups"] == 2 and st["prefix_hit_tokens"] == 32
    assert st["prefill_tokens"] == eng0.stats["prefill_tokens"] - 32 == len(A) + len(B) - 32
    assert eng.runner.paged_prefill_calls == m.cfg.n_layers and eng.runner.gather_prefill_calls == 0
    assert eng0.runner.paged_prefill_calls == 0
    c = eng.runner.cache
    # A registered its two prompt pages at prefill; B adopted them and added none of its own (its third
    # page is partial); at finish nothing new lies wholly below prompt + output - 1 = 43 / 45 tokens
    assert st["prefix_registered_pages"] == 2 and st["prefix_evictions"] == 0
    assert c.free_count() == c.n_pages and sorted(x for x in c.ref if x) == [1, 1]
    c.clear_prefix_index()
    assert not any(c.ref)


def test_engine_hit_with_repetition_penalty_sees_the_prefix():
    m = tiny("gpt-j-6b")
    A, B = _prompts()
    sp = SamplingParams(max_new_tokens=10, repetition_penalty=1.8, do_sample=False)
    want, _, _ = _serve(m, [A, B], [sp, sp])
    got, _, eng = _serve(m, [A, B], [sp, sp], prefix_cache=True)
    assert got == want and eng.stats["prefix_hit_tokens"] == 32
    # the penalty bites: without it the outputs differ, so a `seen` that missed the prefix would show
    plain, _, _ = _serve(m, [A, B], [SamplingParams(max_new_tokens=10, do_sample=False)] * 2)
    assert plain[1] != want[1]
    r = eng.runner
    r.adopt_prefix(0, [], [])
    assert not r.seen[0].any()


def test_engine_hit_with_prefill_chunk():
    """B arrives while A decodes, so its suffix is prefilled in chunks of <= 4 tokens after the adopted pages;
    pages are registered chunk by chunk (a long prompt's third page while it is still prefilling)."""
    m = tiny("gpt-neox-20b")
    A, B = _prompts()
    B = B + [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]  # 49 tokens: a third full page
    sp = SamplingParams(max_new_tokens=6, do_sample=False)
    outs = {}
    for pc in (False, True):
        eng = LLMEngine(m, max_slots=4, max_len=64, page_size=PS, prefill_chunk=4, prefix_cache=pc)
        r0 = eng.generate([A], sp)[0]
        r1 = eng.add_request(A[:20] + [3], SamplingParams(max_new_tokens=30, do_sample=False))
        eng.step()
        r2 = eng.add_request(B, sp)
        seen_registered = []
        while not r2.done:
            eng.step()
            seen_registered.append(eng.stats.get("prefix_registered_pages"))
        eng.run_until_done([r1])
        outs[pc] = (r0.output, r1.output, r2.output)
    assert outs[True] == outs[False]
    assert eng.stats["prefix_hit_tokens"] == 16 + 32 and eng.stats["prefill_chunks"] >= 4
    assert eng.stats["max_step_prefill_tokens"] <= len(A)
    assert seen_registered[0] == 2 and 3 in seen_registered[:-6]  # B's third page: before its first token
    assert eng.runner.gather_prefill_calls == 0 and eng.runner.paged_prefill_calls > 0
    assert eng.runner.cache.free_count() == eng.runner.cache.n_pages


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_engine_hit_with_speculation(mode):
    m = tiny("gpt-j-6b")
    A, B = _prompts()
    sp = SamplingParams(max_new_tokens=12, **(GREEDY if mode == "greedy" else SAMPLED))
    want, why, _ = _serve(m, [A, B], [sp, sp])
    script = Scripted({tuple(A): want[0], tuple(B): want[1]}, wrong=(3,))
    got, why2, eng = _serve(m, [A, B], [sp, sp], prefix_cache=True, spec_tokens=4, proposer=script)
    assert got == want and why2 == why
    assert eng.stats["prefix_hit_tokens"] == 32 and eng.stats["spec_accepted"] > 0


def test_engine_second_turn_hits_pages_registered_at_finish():
    m = tiny("bloom-560m")
    g = torch.Generator().manual_seed(4)
    turn1 = torch.randint(0, VOCAB, (20,), generator=g).tolist()
    sp = SamplingParams(max_new_tokens=14, **SAMPLED)
    eng0 = LLMEngine(m, max_slots=4, max_len=64, page_size=PS)
    eng = LLMEngine(m, max_slots=4, max_len=64, page_size=PS, prefix_cache=True)
    a0, a = eng0.generate([turn1], sp)[0], eng.generate([turn1], sp)[0]
    assert a.output == a0.output and len(a.output) == 14
    # 20 + 14 tokens: position 33 (the last sampled token) was never written, so the pages wholly below it
    # are registered -- one at prefill, the second at finish
    assert eng.stats["prefix_registered_pages"] == 2
    turn2 = turn1 + a.output + [1, 2, 3]
    b0, b = eng0.generate([turn2], sp)[0], eng.generate([turn2], sp)[0]
    assert b.output == b0.output and b.finish_reason == b0.finish_reason
    assert eng.stats["prefix_hit_tokens"] == 32
    # the cap: a prompt of exactly 2 x PS tokens that is fully cached adopts 1 page
    exact = turn2[:2 * PS]
    c0, c = eng0.generate([exact], sp)[0], eng.generate([exact], sp)[0]
    assert c.output == c0.output and eng.stats["prefix_hit_tokens"] == 32 + 16
    assert eng.runner.cache.free_count() == eng.runner.cache.n_pages


def test_engine_window_model_takes_the_gather_loop():
    """GPT-Neo: the local layer (window 8) is outside ``supported`` and keeps the gather loop, the global
    layer runs the paged op; same tokens as without the option."""
    cfg = {"model_type": "gpt_neo", "vocab_size": VOCAB, "hidden_size": 64, "num_layers": 2, "num_heads": 4,
           "attention_types": [[["global", "local"], 1]], "window_size": 8, "max_position_embeddings": 64}
    m = build_model(LMConfig.from_hf(cfg), dtype=torch.float32, seed=0)
    A, B = _prompts(1)
    sp = SamplingParams(max_new_tokens=8, do_sample=False)
    want, _, _ = _serve(m, [A, B], [sp, sp])
    got, _, eng = _serve(m, [A, B], [sp, sp], prefix_cache=True)
    assert got == want and eng.stats["prefix_hit_tokens"] == 32
    assert eng.runner.paged_prefill_calls == 1 and eng.runner.gather_prefill_calls == 1


def test_engine_exact_page_budget_with_a_stale_index():
    """kv_pages = the admitted worst case of one request. Earlier requests leave the pool full of index
    pages; the next request evicts what it needs and ends without KVCacheFull."""
    m = tiny("gpt-j-6b")
    g = torch.Generator().manual_seed(9)
    sp = SamplingParams(max_new_tokens=12, do_sample=False)
    eng = LLMEngine(m, max_slots=2, max_len=64, page_size=PS, kv_pages=4, prefix_cache=True)
    c = eng.runner.cache
    assert c.pages_for(50 + 12) == 4 == c.free_count()
    olds = [torch.randint(0, VOCAB, (50,), generator=g).tolist() for _ in range(2)]
    eng.generate([olds[0]], sp)
    assert len(c.free_pages) == 1 and c.free_count() == 4  # three stale pages, all evictable
    eng.generate([olds[1]], sp)
    assert eng.stats["prefix_evictions"] >= 2 and len(c.free_pages) <= 1
    fresh = torch.randint(0, VOCAB, (50,), generator=g).tolist()
    want = LLMEngine(m, max_slots=2, max_len=64, page_size=PS).generate([fresh], sp)[0].output
    try:
        got = eng.generate([fresh], sp)[0]
    except KVCacheFull as e:  # pragma: no cover
        pytest.fail(str(e))
    assert got.output == want and c.free_count() == 4 and eng._committed == 0
    # two requests in flight share the budget: the second waits for its pages instead of failing
    eng = LLMEngine(m, max_slots=2, max_len=64, page_size=PS, kv_pages=4, prefix_cache=True)
    rs = eng.generate(olds, sp)
    assert all(r.finish_reason == "length" for r in rs) and eng.runner.cache.free_count() == 4


def test_beam_search_neither_looks_up_nor_registers():
    m = tiny("gpt2")
    A, _ = _prompts()
    eng = LLMEngine(m, max_slots=4, max_len=64, page_size=PS, prefix_cache=True)
    want = LLMEngine(m, max_slots=4, max_len=64, page_size=PS).beam_generate(A, 2, 6)
    assert eng.beam_generate(A, 2, 6) == want
    assert eng.stats["prefix_lookups"] == 0 and eng.stats["prefix_registered_pages"] == 0
    assert eng.runner.cache.free_count() == eng.runner.cache.n_pages and not any(eng.runner.cache.ref)


# --------------------------------------------------------------------------------------- options
def test_off_by_default_and_option_values(monkeypatch):
    m = tiny("gpt-j-6b")
    monkeypatch.delenv("KCA_PREFIX_CACHE", raising=False)
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert not eng.prefix_cache and not eng.runner.prefix_cache and eng.runner.cache._pidx is None
    for off in ("0", "off", ""):
        monkeypatch.setenv("KCA_PREFIX_CACHE", off)
        assert not LLMEngine(m, max_slots=2, max_len=32).prefix_cache
    monkeypatch.setenv("KCA_PREFIX_CACHE", "1")
    eng = LLMEngine(m, max_slots=2, max_len=32)
    assert eng.prefix_cache and eng.runner.prefix_cache
    assert not LLMEngine(m, max_slots=2, max_len=32, prefix_cache=False).prefix_cache  # the keyword wins
    monkeypatch.setenv("KCA_PREFIX_CACHE", "maybe")
    with pytest.raises(ValueError, match="KCA_PREFIX_CACHE.*maybe"):
        LLMEngine(m, max_slots=2, max_len=32)
    monkeypatch.delenv("KCA_PREFIX_CACHE")
    runner = ModelRunner(m, max_slots=2, max_len=32, prefix_cache=True)
    assert LLMEngine(m, runner=runner).prefix_cache
    with pytest.raises(ValueError, match="prefix_cache.*runner"):
        LLMEngine(m, runner=runner, prefix_cache=True)
    with pytest.raises(ValueError, match="prefix_cache"):
        ModelRunner(m, max_slots=2, max_len=32).adopt_prefix(0, [], [])


def test_refusals():
    from kubernetes_cloud_amd.parallel.tp_emulation import emulated_rank_model
    m = tiny("gpt-j-6b")
    with pytest.raises(ValueError, match="page_size"):
        LLMEngine(m, max_slots=2, max_len=32, page_size=0, prefix_cache=True)
    with pytest.raises(ValueError, match="fp8"):
        LLMEngine(m, max_slots=2, max_len=32, prefix_cache=True, kv_dtype="fp8")
    cfg = dict(PRESETS_HF["bloom-560m"])
    cfg.update(hidden_size=64, n_layer=2, n_head=4, vocab_size=96)
    tp = emulated_rank_model(LMConfig.from_hf(cfg), 2, 0, dtype=torch.float32)
    with pytest.raises(ValueError, match="tensor-parallel"):
        LLMEngine(tp, max_slots=2, max_len=32, prefix_cache=True)
    split = tiny("gpt-j-6b")
    split.h[1].to("meta")  # a second device under the last layer: a layer-split placement
    with pytest.raises(ValueError, match="layer-split"):
        LLMEngine(split, max_slots=2, max_len=32, prefix_cache=True)
    with pytest.raises(ValueError, match="paged"):
        KVCache(1, 2, 1, 32, 8, "cpu", torch.float32, page_size=0).enable_prefix_index()
