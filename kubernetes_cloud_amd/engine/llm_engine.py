"""Continuous-batching LLM engine over ``ModelRunner``.

Replaces what the reference delegates to FasterTransformer-on-Triton
(online-inference/fastertransformer), DeepSpeed-Inference
(bloom-176b-deepspeed) and HF ``pipeline``/``generate`` (inference.py:67-96,
bloom.py:57-77, kserve_api.py:47-72): requests join and leave the running batch
every step (iteration-level scheduling), each request owns one KV-cache slot,
sampling parameters are per request (FT's per-request runtime_top_k / top_p /
temperature / repetition_penalty / random_seed / bad_words / stop_words /
output log-probs).

``step()`` = admit waiting requests (prefill + first token) while slots and
KV pages are free, then one fused decode step for every running request.
One-step lookahead (``pipeline``, on with a pipelining runner): a step launches
the next decode -- its input tokens chained on the device from the step in
flight (``ModelRunner.decode_async``) -- and only then reads the in-flight
step's tokens, so stop checks, streaming callbacks and row preparation overlap
the GPU instead of idling it. A request that stops on a token the host has not
seen yet gets one discarded extra token computed; length stops are predicted
and never over-run.
Chunked prefill (``prefill_chunk``): while requests are decoding, a step
spends at most ``prefill_chunk`` prompt tokens on prefill -- a long prompt is
prefilled over several steps (``ModelRunner.prefill(..., start=)`` continues
its slot), each followed by the decode step of the running batch, so a
2048-token admission no longer stalls every running stream for its whole
prefill; with nothing decoding a prompt prefills in one pass.
Admission reserves a request's worst-case page count (prompt + max_new_tokens)
against the paged cache, so a running request never runs out of pages (no
preemption needed); pages go back to the pool the step a request finishes.
Admitted prompts of different lengths prefill together, right-padded into a
few length-sorted batches (``_prefill_groups``).
Speculative decoding (``spec_tokens=T``, or ``KCA_DECODE_SPEC=T`` in the environment; off by default):
every step a proposer (``engine.spec.NgramProposer`` unless one is given) drafts up to T - 1 tokens per
running request and ``ModelRunner.verify`` samples all T positions in one pass over the weights. With
samples s_0..s_{n-1} of drafts d_1..d_{n-1} the request takes s_0, then s_t while s_{t-1} == d_t: each
token is sampled from the model's own distribution given a prefix that is already confirmed, with the
seed and the bans of its position, so greedy and seeded sampled outputs are what they are without
speculation. Drafts never reach past the request's ``max_new_tokens`` / ``max_len``, so the admission's
page count stays exact. A request with a repetition penalty or a multi-token bad word, or without a
proposal, rides along with one token; a step in which nobody has a draft is an ordinary decode step.
The one-step lookahead is off while speculation is on.
Quantized-weight prefill (``prefill_weights="quantized"``, or ``KCA_PREFILL_WEIGHTS=quantized`` in the
environment; off by default; needs ``weight_dtype``): prefill runs on the quantized weights as decode does and
the runner releases the 16-bit weights of the quantized projections (engine/runner.py) -- one model per
request, and the memory the quantization was for. Composes with ``kv_dtype="fp8"`` and ``spec_tokens``.
Prefix caching (``prefix_cache=True``, or ``KCA_PREFIX_CACHE=1`` in the environment; off by default; paged
cache only): requests share the KV pages of a common prompt prefix -- a system prompt, a few-shot block,
the earlier turns of a chat. A page is registered in the cache's index (``KVCache``) once prefill has
written all of its positions (per chunk under ``prefill_chunk``), and when a request finishes the pages
lying wholly below ``len(prompt) + len(output) - 1`` follow (the last sampled token's K/V may never have
been written), so the next turn of a conversation hits. Admission takes the longest registered chain of
full pages of the prompt, at most ``(len(prompt) - 1) // PS`` pages -- at least one token is computed, for
its logits -- adopts it (``ModelRunner.adopt_prefix``) and prefills only the rest; hits and misses batch
together, grouped by the length still to compute. Admission control is unchanged: every request commits
its worst case in full, so the pages in use never exceed the commitment and free plus evictable pages
always cover it; index pages nobody uses are evicted, least recently used first, when the free list runs
short. ``beam_generate`` neither looks up nor registers. ``stats``: ``prefix_lookups``,
``prefix_hit_tokens``, ``prefix_registered_pages``, ``prefix_evictions``; ``prefill_tokens`` counts computed
tokens only.
``start()`` runs
the loop on a background thread for the HTTP servers; ``generate()`` is the
synchronous batch API used by the finetuner sampler and the evaluator.
"""
from __future__ import annotations

import dataclasses
import itertools
import random
import threading
import time
from concurrent.futures import Future

import torch

from .runner import ModelRunner, mix_seed


@dataclasses.dataclass
class SamplingParams:
    max_new_tokens: int = 50
    min_new_tokens: int = 0
    do_sample: bool = True
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    seed: int | None = None
    eos_token_id: int | None = None
    stop_sequences: list | None = None   # list of token-id lists (FT stop_words_list)
    bad_words_ids: list | None = None    # list of token-id lists (FT bad_words_list / HF bad_words_ids)
    logprobs: bool = False


@dataclasses.dataclass
class Request:
    rid: int
    prompt: list
    params: SamplingParams
    output: list = dataclasses.field(default_factory=list)
    logprobs: list = dataclasses.field(default_factory=list)
    finish_reason: str | None = None
    slot: int = -1
    seed: int = 0
    t_arrive: float = 0.0
    t_first: float = 0.0
    t_done: float = 0.0
    future: Future | None = None
    on_token: object = None  # callable(request) after every generated token (streaming front ends)
    prefilled: int = 0       # chunked prefill: prompt tokens already in the KV cache

    @property
    def done(self) -> bool:
        return self.finish_reason is not None

    @property
    def tokens(self) -> list:
        return self.prompt + self.output


class LLMEngine:
    def __init__(self, model, max_slots: int = 32, max_len: int | None = None, use_graphs: bool | None = None,
                 max_prefill_tokens: int = 16384, runner=None, page_size: int | None = None,
                 kv_pages: int | None = None, prefill_chunk: int | None = None, pipeline: bool | None = None,
                 weight_dtype: str | None = None, kv_dtype: str | None = None,
                 spec_tokens: int | str | None = None, proposer=None, prefill_weights: str | None = None,
                 prefix_cache: bool | str | None = None):
        # ``spec_tokens=T`` (2 / 4 / 8): speculative decoding (module docstring; None reads KCA_DECODE_SPEC);
        # ``proposer``: an object with ``propose(tokens, k) -> list[int]`` (default: engine.spec.NgramProposer)
        # ``weight_dtype="fp8"`` / ``"mxfp4"``: FP8 / MXFP4 weight-only decode (engine/runner.py; None reads
        # KCA_DECODE_WEIGHTS)
        # ``kv_dtype="fp8"``: FP8 KV cache (engine/runner.py; None reads KCA_DECODE_KV)
        # ``prefill_weights="quantized"``: prefill on the quantized weights, 16-bit projection weights released
        # (engine/runner.py; None reads KCA_PREFILL_WEIGHTS)
        # ``prefix_cache=True``: requests share the KV pages of a common prompt prefix (module docstring; None
        # reads KCA_PREFIX_CACHE)
        # ``runner``: e.g. a tp_driver.CollectiveRunner that mirrors every call to TP follower ranks
        if runner is not None and weight_dtype is not None:
            raise ValueError("weight_dtype applies to the runner the engine builds; a supplied runner sets its own")
        if runner is not None and kv_dtype is not None:
            raise ValueError("kv_dtype applies to the runner the engine builds; a supplied runner sets its own")
        if runner is not None and spec_tokens is not None:
            raise ValueError("spec_tokens applies to the runner the engine builds; a supplied runner sets its own")
        if runner is not None and prefill_weights is not None:
            raise ValueError("prefill_weights applies to the runner the engine builds; a supplied runner sets its own")
        if runner is not None and prefix_cache is not None:
            raise ValueError("prefix_cache applies to the runner the engine builds; a supplied runner sets its own")
        self.runner = runner or ModelRunner(model, max_slots=max_slots, max_len=max_len, use_graphs=use_graphs,
                                            page_size=page_size, kv_pages=kv_pages, weight_dtype=weight_dtype,
                                            kv_dtype=kv_dtype, spec_tokens=spec_tokens,
                                            prefill_weights=prefill_weights, prefix_cache=prefix_cache)
        self.spec_tokens = int(getattr(self.runner, "spec_tokens", 0) or 0)
        if self.spec_tokens and pipeline:
            raise ValueError("pipeline=True (one-step lookahead) does not combine with speculative decoding")
        if proposer is not None and not callable(getattr(proposer, "propose", None)):
            raise ValueError("proposer needs a propose(tokens, k) -> list[int] method")
        if self.spec_tokens and proposer is None:
            from .spec import NgramProposer
            proposer = NgramProposer()
        self.proposer = proposer
        max_slots = self.runner.max_slots
        self.max_len = self.runner.max_len
        self.free = list(range(max_slots))[::-1]
        self.waiting: list[Request] = []
        self.running: list[Request] = []
        self._ids = itertools.count()
        self._lock = threading.Lock()
        self._step_lock = threading.Lock()
        self._wake = threading.Event()
        self._thread = None
        self._stop = False
        self.max_prefill_tokens = max_prefill_tokens
        # prompt-token budget of a step while requests are decoding (None/0: whole prompts)
        self.prefill_chunk = int(prefill_chunk) if prefill_chunk else 0
        self.prefilling: list[Request] = []  # admitted, prompt partially in the cache (r.prefilled tokens)
        self.pipeline = bool(getattr(self.runner, "pipelined", False)) if pipeline is None else pipeline
        if self.spec_tokens:
            self.pipeline = False
        self._inflight = None  # (DecodeHandle, [Request]) of the launched, not yet read decode step
        self.stats = {"steps": 0, "decode_tokens": 0, "prefill_tokens": 0, "finished": 0, "prefill_batches": 0,
                      "prefill_pad_tokens": 0, "prefill_chunks": 0, "max_step_prefill_tokens": 0,
                      "decode_steps": 0, "spec_steps": 0, "spec_drafted": 0, "spec_accepted": 0}
        cache = getattr(self.runner, "cache", None)
        # prefix caching (module docstring): only with a runner of this process (a CollectiveRunner's
        # followers keep caches of their own)
        self.prefix_cache = isinstance(self.runner, ModelRunner) and bool(self.runner.prefix_cache)
        if self.prefix_cache:
            self.stats.update(prefix_lookups=0, prefix_hit_tokens=0, prefix_registered_pages=0, prefix_evictions=0)
        self._paged = cache is not None and getattr(cache, "paged", False)
        self._page_budget = cache.n_pages if self._paged else 0
        self._committed = 0  # worst-case pages promised to admitted requests

    # ------------------------------------------------------------ requests
    def add_request(self, prompt: list, params: SamplingParams, future: Future | None = None,
                    on_token=None) -> Request:
        prompt = [int(t) for t in prompt]
        if not prompt:
            raise ValueError("empty prompt")
        if len(prompt) >= self.max_len:
            prompt = prompt[-(self.max_len - 1):]
        seed = params.seed if params.seed is not None else random.getrandbits(63)
        r = Request(next(self._ids), prompt, params, seed=seed, t_arrive=time.perf_counter(), future=future,
                    on_token=on_token)
        if params.max_new_tokens <= 0:
            r.finish_reason = "length"
            r.t_done = r.t_arrive
            if future is not None:
                future.set_result(r)
            return r
        with self._lock:
            self.waiting.append(r)
        self._wake.set()
        return r

    def has_work(self) -> bool:
        return bool(self.waiting or self.running or self.prefilling or self._inflight)

    def _row(self, r: Request, token: int | None = None, ahead: int = 0) -> dict:
        """Decode-row parameters. ``ahead`` = 1: the row's input token is the
        in-flight step's (not yet on the host), chained on the device."""
        p = r.params
        n_gen = len(r.output) + ahead
        greedy = (not p.do_sample) or p.temperature <= 0
        bans = []
        for w in p.bad_words_ids or ():
            if len(w) == 1:
                bans.append(int(w[0]))
            elif len(w) > 1 and r.tokens[-(len(w) - 1):] == list(w[:-1]):
                bans.append(int(w[-1]))
        if p.eos_token_id is not None and n_gen < p.min_new_tokens:
            bans.append(int(p.eos_token_id))
        if ahead:
            return {"token": None, "pos": len(r.tokens) - 1 + ahead,
                    "slot": r.slot, "temperature": 0.0 if greedy else float(p.temperature),
                    "top_k": int(p.top_k or 0), "top_p": float(p.top_p if p.top_p is not None else 1.0),
                    "rep": float(p.repetition_penalty or 1.0), "seed": mix_seed(r.seed, n_gen), "bans": bans}
        return {"token": token if token is not None else r.tokens[-1], "pos": len(r.tokens) - 1,
                "slot": r.slot, "temperature": 0.0 if greedy else float(p.temperature),
                "top_k": int(p.top_k or 0), "top_p": float(p.top_p if p.top_p is not None else 1.0),
                "rep": float(p.repetition_penalty or 1.0), "seed": mix_seed(r.seed, n_gen), "bans": bans}

    def _append(self, r: Request, tok: int, lp: float):
        r.output.append(int(tok))
        if r.params.logprobs:
            r.logprobs.append(float(lp))
        p = r.params
        if len(r.output) == 1:
            r.t_first = time.perf_counter()
        if p.eos_token_id is not None and tok == p.eos_token_id and len(r.output) > p.min_new_tokens:
            r.finish_reason = "stop"
        elif any(s and r.output[-len(s):] == list(s) for s in (p.stop_sequences or ())):
            r.finish_reason = "stop"
        elif len(r.output) >= p.max_new_tokens or len(r.tokens) >= self.max_len:
            r.finish_reason = "length"
        if r.on_token is not None:
            try:
                r.on_token(r)
            except Exception:  # noqa: BLE001 -- a broken stream consumer must not stall the batch
                r.on_token = None

    def _pages_needed(self, r: Request) -> int:
        if not self._paged:
            return 0
        return self.runner.cache.pages_for(min(len(r.prompt) + r.params.max_new_tokens, self.max_len))

    def _free_slot(self, r: Request):
        if r.slot >= 0:
            self.runner.release(r.slot)
            self.free.append(r.slot)
            r.slot = -1
            self._committed -= self._pages_needed(r)

    def _register(self, r: Request, n_tokens: int):
        """Prefix caching: the pages of ``r`` lying wholly below position ``n_tokens`` into the index."""
        if self.prefix_cache and r.slot >= 0:
            cache = self.runner.cache
            cache.register(r.slot, r.tokens, n_tokens // cache.page_size)
            self.stats["prefix_registered_pages"] = cache.prefix_registered

    def _lookup(self, r: Request):
        """Prefix caching: adopt the longest cached chain of full pages of ``r``'s prompt into its slot."""
        cache = self.runner.cache
        pages = cache.lookup(r.prompt, (len(r.prompt) - 1) // cache.page_size)
        self.stats["prefix_lookups"] += 1
        if pages:
            r.prefilled = len(pages) * cache.page_size
            self.runner.adopt_prefix(r.slot, pages, r.prompt[:r.prefilled])
            self.stats["prefix_hit_tokens"] += r.prefilled

    def _finish(self, r: Request):
        r.t_done = time.perf_counter()
        self._register(r, len(r.tokens) - 1)  # (the last sampled token's K/V may never have been written)
        self._free_slot(r)
        self.stats["finished"] += 1
        if r.future is not None and not r.future.done():
            r.future.set_result(r)

    # ---------------------------------------------------------------- step
    def beam_generate(self, prompt: list, num_beams: int, max_new_tokens: int, eos_token_id: int | None = None,
                      len_penalty: float = 1.0, diversity_rate: float = 0.0, n_return: int = 1):
        """Beam search for one prompt on ``num_beams`` slots of this engine's cache
        (mutually exclusive with ``step``; FT beam_width > 1 requests)."""
        from .beam import beam_search
        # a tensor-parallel runner (tp_driver.CollectiveRunner) mirrors prefill / decode_topk /
        # copy_slots / release to its followers, so beams run under TP unchanged
        need = 0
        if self._paged:
            need = num_beams * (self.runner.cache.pages_for(min(len(prompt) + max_new_tokens, self.max_len)) + 1)
        with self._step_lock:
            self._drain([])  # the in-flight lookahead step finishes before the beams take the runner
            with self._lock:
                if len(self.free) < num_beams:
                    raise RuntimeError(f"need {num_beams} free cache slots, have {len(self.free)}")
                if self._committed + need > self._page_budget and self._paged:
                    raise RuntimeError(f"need {need} free KV pages, have {self._page_budget - self._committed}")
                slots = [self.free.pop() for _ in range(num_beams)]
                self._committed += need
            try:
                return beam_search(self.runner, [int(t) for t in prompt], slots, max_new_tokens, eos_token_id,
                                   len_penalty, diversity_rate, n_return)
            finally:
                with self._lock:
                    for s_ in slots:
                        self.runner.release(s_)
                    self.free.extend(slots)
                    self._committed -= need

    def step(self) -> list[Request]:
        """Admit + one decode step. Returns the requests that finished."""
        with self._step_lock:
            return self._step()

    def _first_token(self, r: Request, logits, finished: list):
        toks, lps = self.runner.sample_first(logits, [self._row(r, 0)])
        self._append(r, toks[0], lps[0])
        if r.done:
            self._finish(r)
            finished.append(r)
        else:
            self.running.append(r)

    def _chunk_step(self, budget: int, finished: list) -> int:
        """Advance partially prefilled prompts by up to ``budget`` tokens."""
        used = 0
        for r in list(self.prefilling):
            if used >= budget:
                break
            p0 = r.prefilled
            n = min(budget - used, len(r.prompt) - p0)
            ids = torch.tensor([r.prompt[p0:p0 + n]], dtype=torch.long)
            logits = self.runner.prefill(ids, [r.slot], [n], start=[p0])
            r.prefilled += n
            self._register(r, r.prefilled)
            used += n
            self.stats["prefill_tokens"] += n
            self.stats["prefill_chunks"] += 1
            if r.prefilled == len(r.prompt):
                self.prefilling.remove(r)
                self._first_token(r, logits, finished)
        return used

    def _step(self) -> list[Request]:
        finished = []
        chunked = self.prefill_chunk > 0 and (self.running or self.prefilling)
        budget = self.prefill_chunk if chunked else self.max_prefill_tokens
        used = self._chunk_step(budget, finished) if self.prefilling else 0
        budget -= used
        with self._lock:
            admit = []
            while self.waiting and self.free and budget > 0 and (not admit or budget >= len(self.waiting[0].prompt)):
                need = self._pages_needed(self.waiting[0])
                if self._paged and self._committed + need > self._page_budget:
                    if need > self._page_budget:  # can never fit: fail it rather than block the queue
                        r = self.waiting.pop(0)
                        r.finish_reason = "error"
                        r.t_done = time.perf_counter()
                        if r.future is not None and not r.future.done():
                            r.future.set_exception(RuntimeError(
                                f"request needs {need} KV pages > cache size {self._page_budget}"))
                        continue
                    break
                r = self.waiting.pop(0)
                r.slot = self.free.pop()
                self._committed += need
                r.prefilled = 0
                if self.prefix_cache:
                    self._lookup(r)
                if chunked and len(r.prompt) - r.prefilled > budget:  # prefill this one chunk by chunk
                    self.prefilling.append(r)
                    break
                budget -= len(r.prompt) - r.prefilled
                admit.append(r)
        if self.prefilling and budget > 0 and chunked:
            used += self._chunk_step(budget, finished)
        for group in _prefill_groups(admit):
            # (prefix caching: r.prefilled tokens of the prompt are adopted pages; the rest is computed)
            start = [r.prefilled for r in group]
            lens = [len(r.prompt) - r.prefilled for r in group]
            T = max(lens)
            ids = torch.tensor([r.prompt[r.prefilled:] + [0] * (T - L) for r, L in zip(group, lens)],
                               dtype=torch.long)
            if any(start):
                logits = self.runner.prefill(ids, [r.slot for r in group], lens, start=start)
            elif all(L == T for L in lens):
                logits = self.runner.prefill(ids, [r.slot for r in group])
            else:
                logits = self.runner.prefill(ids, [r.slot for r in group], lens)
            for r in group:
                r.prefilled = len(r.prompt)
                self._register(r, r.prefilled)
            toks, lps = self.runner.sample_first(logits, [self._row(r, 0) for r in group])
            self.stats["prefill_tokens"] += sum(lens)
            used += sum(lens)
            self.stats["prefill_pad_tokens"] += T * len(group) - sum(lens)
            self.stats["prefill_batches"] += 1
            for r, t, lp in zip(group, toks, lps):
                self._append(r, t, lp)
                if r.done:
                    self._finish(r)
                    finished.append(r)
                else:
                    self.running.append(r)
        # decode one token for everything already running (incl. just admitted)
        if self.pipeline and self._lookahead_ok():
            self._decode_lookahead(finished)
        elif self.running or self._inflight:
            self._drain(finished)
            # the drained step may have finished requests (slot released, pages freed)
            self.running = [r for r in self.running if not r.done]
            rows = [self._row(r) for r in self.running]
            if rows and self.spec_tokens and self._decode_spec(rows, finished):
                pass
            elif rows:
                toks, lps = self.runner.decode(rows)
                self.stats["decode_tokens"] += len(rows)
                self.stats["decode_steps"] += 1
                self._take(self.running, toks, lps, finished)
            self.running = [r for r in self.running if not r.done]
        if self.prefix_cache:
            self.stats["prefix_evictions"] = self.runner.cache.prefix_evictions
        self.stats["steps"] += 1
        self.stats["max_step_prefill_tokens"] = max(self.stats["max_step_prefill_tokens"], used)
        return finished

    # ------------------------------------------------------------ lookahead
    def _take(self, reqs, toks, lps, finished):
        for r, t, lp in zip(reqs, toks, lps):
            if r.done:  # stopped on the previous token: this one was computed ahead and is dropped
                continue
            self._append(r, t, lp)
            if r.done:
                self._finish(r)
                finished.append(r)

    # ---------------------------------------------------------- speculation
    def _drafts(self, r: Request) -> list:
        """Up to T - 1 drafted tokens for ``r``: none for a request the verify step does not cover, and
        never more than it may still generate after this step's own token."""
        p = r.params
        k = min(self.spec_tokens - 1, p.max_new_tokens - len(r.output) - 1, self.max_len - len(r.tokens) - 1)
        if k <= 0 or (p.repetition_penalty or 1.0) != 1.0 or any(len(w) > 1 for w in (p.bad_words_ids or ())):
            return []
        return [int(t) for t in self.proposer.propose(r.tokens, k)][:k]

    def _decode_spec(self, rows: list, finished) -> bool:
        """Draft and verify for the running requests (``rows``: their decode rows). False -- nothing
        launched -- when no request has a draft: the caller runs the ordinary decode step."""
        drafts = [self._drafts(r) for r in self.running]
        if not any(drafts):
            return False
        vrows = []
        for r, row, d in zip(self.running, rows, drafts):
            p, n_gen = r.params, len(r.output)
            single = [int(w[0]) for w in (p.bad_words_ids or ()) if len(w) == 1]
            bans = [row["bans"]]
            for t in range(1, len(d) + 1):  # position t's own bans: it is the (n_gen + t)-th new token
                eos = p.eos_token_id is not None and n_gen + t < p.min_new_tokens
                bans.append(single + ([int(p.eos_token_id)] if eos else []))
            vrows.append({"tokens": [row["token"]] + d, "pos": row["pos"], "slot": row["slot"],
                          "temperature": row["temperature"], "top_k": row["top_k"], "top_p": row["top_p"],
                          "rep": row["rep"], "seeds": [mix_seed(r.seed, n_gen + t) for t in range(len(d) + 1)],
                          "bans": bans})
        ids, lps = self.runner.verify(vrows)
        self.stats["decode_steps"] += 1
        self.stats["spec_steps"] += 1
        for r, d, s, lp in zip(self.running, drafts, ids, lps):
            self.stats["spec_drafted"] += len(d)
            for t in range(len(s)):
                if t > 0 and s[t - 1] != d[t - 1]:
                    break  # draft t was wrong: sample t was drawn after a token the request does not have
                self._append(r, s[t], lp[t])
                self.stats["decode_tokens"] += 1
                self.stats["spec_accepted"] += t > 0
                if r.done:
                    self._finish(r)
                    finished.append(r)
                    break
        return True

    def _drain(self, finished):
        """Read the in-flight decode step (before a synchronous runner call)."""
        if self._inflight is not None:
            h, reqs = self._inflight
            self._inflight = None
            toks, lps = h.result()
            self._take(reqs, toks, lps, finished)

    def _lookahead_ok(self) -> bool:
        # a multi-token bad word's ban depends on the token still in flight
        return not any(len(w) > 1 for r in self.running for w in (r.params.bad_words_ids or ()))

    def _last_by_length(self, r: Request, ahead: int) -> bool:
        return (len(r.output) + ahead >= r.params.max_new_tokens
                or len(r.tokens) + ahead >= self.max_len)

    def _decode_lookahead(self, finished):
        """Launch step t+1 (tokens of step t chained on the device), then read step t."""
        inflight = self._inflight
        src = {id(r): i for i, r in enumerate(inflight[1])} if inflight else {}
        rows, reqs = [], []
        for r in self.running:
            if r.done:
                continue
            j = src.get(id(r))
            if j is None:
                rows.append(self._row(r))
            else:
                if self._last_by_length(r, 1):  # its in-flight token is its last one
                    continue
                row = self._row(r, ahead=1)
                row["src"] = j
                rows.append(row)
            reqs.append(r)
        h = self.runner.decode_async(rows, prev=inflight[0] if inflight else None) if rows else None
        if rows:
            self.stats["decode_tokens"] += len(rows)
            self.stats["decode_steps"] += 1
        self._inflight = None
        if inflight is not None:
            toks, lps = inflight[0].result()
            self._take(inflight[1], toks, lps, finished)
        self._inflight = (h, reqs) if h is not None else None
        self.running = [r for r in self.running if not r.done]

    def run_until_done(self, reqs: list[Request] | None = None):
        while self.has_work() and (reqs is None or not all(r.done for r in reqs)):
            self.step()

    def generate(self, prompts: list[list[int]], params: SamplingParams | list[SamplingParams]) -> list[Request]:
        ps = params if isinstance(params, list) else [params] * len(prompts)
        reqs = [self.add_request(p, sp) for p, sp in zip(prompts, ps)]
        self.run_until_done(reqs)
        return reqs

    # ------------------------------------------------------ background loop
    def submit(self, prompt: list, params: SamplingParams, on_token=None) -> Future:
        if self._thread is None:
            self.start()
        fut: Future = Future()
        self.add_request(prompt, params, fut, on_token=on_token)
        return fut

    def start(self):
        if self._thread is not None:
            return
        self._stop = False
        self._thread = threading.Thread(target=self._loop, name="llm-engine", daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        self._wake.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None

    def _loop(self):
        dev = self.runner.device
        if dev.type == "cuda":
            torch.cuda.set_device(dev)
        while not self._stop:
            if not self.has_work():
                self._wake.wait(0.05)
                self._wake.clear()
                continue
            try:
                self.step()
            except Exception as e:  # fail every in-flight request, keep serving
                with self._lock:
                    victims = self.running + self.prefilling + self.waiting
                    self.running, self.prefilling, self.waiting = [], [], []
                    self._inflight = None
                for r in victims:
                    try:
                        self._free_slot(r)
                    except Exception:  # noqa: BLE001 -- a broken runner must not stop the loop
                        r.slot = -1
                    if r.future is not None and not r.future.done():
                        r.future.set_exception(e)


def _prefill_groups(reqs: list[Request], slack: float = 0.25, min_slack: int = 256) -> list[list[Request]]:
    """Length-sorted batches whose right padding stays within ``slack`` of the
    real tokens (or ``min_slack`` tokens: short prompts are launch-bound, so
    they batch freely). The length is what prefill computes: the prompt less
    the ``prefilled`` tokens a prefix-cache hit adopted."""
    out, cur, real = [], [], 0
    for r in sorted(reqs, key=lambda r: len(r.prompt) - r.prefilled):
        L = len(r.prompt) - r.prefilled
        if cur and L * (len(cur) + 1) - (real + L) > max(slack * (real + L), min_slack):
            out.append(cur)
            cur, real = [], 0
        cur.append(r)
        real += L
    if cur:
        out.append(cur)
    return out


__all__ = ["LLMEngine", "SamplingParams", "Request"]
