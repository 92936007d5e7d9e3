#!/usr/bin/env python3
"""Speculative decoding A/B (ops/spec.py, csrc/kernels/decode_spec.hip, engine/spec.py).

Two tables, one JSON line per row, appended to ``--out``; bench/kv8_bench.py's protocol (one process, the
arms alternating repetition by repetition, >= 20 repetitions, each a pass over >= 1 GiB of distinct paged
caches replayed as one HIP graph, median (min..max)):

* kernel: the attention of a verify step over T tokens per sequence, three arms --
    spec    ``spec_prep_attention`` on B x T rows (prep + attention + combine launches);
    rows    ``decode_prep`` + ``decode_attention`` on B x T rows, row (b, t) a sequence of its own length
            (the kernels a tree without the multi-token kernel would use; two launches, since the fused
            one-launch kernel cannot serve rows that read each other's appended K/V);
    single  ``decode_prep_attention`` on B rows: the ordinary decode step's attention, one token each --
  at the head shapes of GPT-J (16 x 256), GPT-NeoX-20B (64 x 96) and a BLOOM-176B TP=8 rank (14 x 128,
  ALiBi), B = 1 / 8 sequences of 512 / 2048 / 8192 cached tokens, T = 2 / 4 / 8.
* engine: ``LLMEngine`` with HIP graphs on random-init weights (as bench/decode_bench.py builds them),
  prompts of 512 tokens: ms per plain decode step against ms per verify step for T = 2 / 4 / 8 under a
  scripted proposer that is always right (acceptance 1: T tokens per step) and one that is always wrong
  (acceptance 0: one token per step at the verify step's price), tokens/s of both, the break-even
  acceptance (verify_ms / decode_ms - 1) / (T - 1), and the host time of the proposers per step
  (the scripted one as run, and ``NgramProposer`` on the same token lists).

Needs a GPU; reads nothing outside the repository.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# local heads, KV heads, head dim, rotary dims, interleaved, ALiBi (bench/kv8_bench.py's shapes)
SHAPES = {
    "gpt-j-6b": dict(H=16, Hkv=16, D=256, rot=64, inter=True, alibi=False),
    "gpt-neox-20b": dict(H=64, Hkv=64, D=96, rot=24, inter=False, alibi=False),
    "bloom-176b-tp8-rank": dict(H=14, Hkv=14, D=128, rot=0, inter=False, alibi=True),
}
ROTATE_BYTES = 1 << 30
PS = 64


def _emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def _stats(xs, nd=2):
    return round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)


def kernel_table(fh, reps: int, models, batches, kvs, Ts, max_buffers: int):
    from kubernetes_cloud_amd.ops import decode as dops
    from kubernetes_cloud_amd.ops import spec
    from kubernetes_cloud_amd.ops.rope import rope_tables
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = lambda xs: torch.tensor(xs, device=dev, dtype=torch.int32)  # noqa: E731
    for model in models:
        s = SHAPES[model]
        H, Hkv, D, rot = s["H"], s["Hkv"], s["D"], s["rot"]
        for B in batches:
            for kv in kvs:
                nb = kv // PS
                pages = B * nb
                b16 = B * Hkv * kv * 2 * D * 2  # K + V bytes one pass over the B sequences streams
                nbuf = min(max_buffers, max(2, -(-ROTATE_BYTES // b16)))
                tbl = torch.randperm(pages, generator=torch.Generator().manual_seed(kv + B)).view(B, nb)
                tbl = tbl.to(torch.int32).to(dev)
                shape = (pages + 1, Hkv, PS, D)
                caches = [tuple(torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16) for _ in "kv")
                          for _ in range(nbuf)]
                cos, sin = rope_tables(rot, kv, 10000.0, dev) if rot else (None, None)
                al = (2.0 ** (-8.0 * torch.arange(1, H + 1, device=dev) / H)).float() if s["alibi"] else None
                scale = D ** -0.5
                slots = torch.arange(B, device=dev, dtype=torch.int32)
                for T in Ts:
                    M = B * T
                    qkv = torch.randn(M, (H + 2 * Hkv) * D, generator=g, device=dev).to(torch.bfloat16)
                    out = torch.empty(M, H * D, device=dev, dtype=torch.bfloat16)
                    base, n_tok, lens = i32([kv - T] * B), i32([T] * B), i32([kv] * B)
                    row_pos = i32([kv - T + t for _ in range(B) for t in range(T)])
                    row_slots = i32([b for b in range(B) for _ in range(T)])
                    row_lens = row_pos + 1
                    one_pos, one_lens = i32([kv - 1] * B), i32([kv] * B)
                    ws = {k: torch.zeros(max(n, 1), device=dev, dtype=torch.float32) for k, n in (
                        ("spec", spec.spec_ws_floats(B, T, H, Hkv, D, kv)), ("rows", dops.decode_ws_floats(M, H, Hkv, D, kv)),
                        ("single", dops.decode_ws_floats(B, H, Hkv, D, kv)))}

                    def arm_spec(i):  # (Q is re-rotated in place call after call: same work, finite values)
                        spec.spec_prep_attention(qkv, H, Hkv, D, rot, s["inter"], cos, sin, base, n_tok, slots, T,
                                                 caches[i][0], caches[i][1], lens, kv, scale, al, out=out,
                                                 ws=ws["spec"], block_table=tbl)

                    def arm_rows(i):
                        dops.decode_prep(qkv, H, Hkv, D, rot, s["inter"], cos, sin, row_pos, row_slots, caches[i][0],
                                         caches[i][1], tbl)
                        dops.decode_attention(qkv, caches[i][0], caches[i][1], row_slots, row_lens, H, kv, scale, al,
                                              out=out, ws=ws["rows"], block_table=tbl)

                    def arm_single(i):
                        dops.decode_prep_attention(qkv[:B], H, Hkv, D, rot, s["inter"], cos, sin, one_pos, slots,
                                                   caches[i][0], caches[i][1], one_lens, kv, scale, al, out=out[:B],
                                                   ws=ws["single"], block_table=tbl)

                    def as_graph(fn):  # one pass over the buffers as one HIP graph: what the engine replays
                        side = torch.cuda.Stream()
                        side.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(side):
                            for i in range(nbuf):
                                fn(i)
                        torch.cuda.current_stream().wait_stream(side)
                        gr = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gr):
                            for i in range(nbuf):
                                fn(i)
                        return gr

                    def one_pass(gr):
                        s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s0.record()
                        gr.replay()
                        e0.record()
                        e0.synchronize()
                        return s0.elapsed_time(e0) / nbuf * 1e3  # us per call

                    graphs = {"spec": as_graph(arm_spec), "rows": as_graph(arm_rows), "single": as_graph(arm_single)}
                    for _ in range(2):
                        for gr in graphs.values():
                            one_pass(gr)
                    ts = {k: [] for k in graphs}
                    for _ in range(reps):
                        for k, gr in graphs.items():
                            ts[k].append(one_pass(gr))
                    row = {"table": "kernel", "model": model, "B": B, "kv": kv, "T": T, "H": H, "D": D, "page": PS,
                           "reps": reps, "timing": "hip graph replay", "buffers": nbuf,
                           "rotated_MiB": round(nbuf * b16 / 2 ** 20), "chunk": dops.decode_chunk(B, Hkv, kv)}
                    for k in graphs:
                        md, lo, hi = _stats(ts[k])
                        row.update({f"{k}_us": md, f"{k}_us_min": lo, f"{k}_us_max": hi})
                    row["spec_GBps"] = round(b16 / row["spec_us"] / 1e3, 1)
                    row["rows_over_spec"] = round(row["rows_us"] / row["spec_us"], 3)
                    row["spec_over_single"] = round(row["spec_us"] / row["single_us"], 3)
                    # the arms' spreads overlap: no winner at this shape
                    row["spec_beats_rows"] = bool(row["spec_us_max"] < row["rows_us_min"])
                    _emit(fh, row)
                    del graphs
                del caches
                torch.cuda.empty_cache()


class Oracle:
    """Scripted proposer: drafts the known continuation of each prompt -- right (``wrong=False``) or with
    every token off by one (``wrong=True``: the first draft is always rejected). Times itself."""

    def __init__(self, vocab: int, wrong: bool):
        self.scripts, self.vocab, self.wrong, self.seconds, self.calls = {}, vocab, wrong, 0.0, 0

    def propose(self, tokens, k):
        t0 = time.perf_counter()
        out = []
        for p, full in self.scripts.items():
            n = len(p)
            if len(tokens) > n and tuple(tokens[:n]) == p:
                i = len(tokens) - n
                if tokens[n:] == full[:i]:
                    out = full[i:i + k]
                    if self.wrong:
                        out = [(t + 1) % self.vocab for t in out]
                break
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        return out


def engine_table(fh, model: str, batches, Ts, prompt_len: int, reps: int, new_tokens: int):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.engine.spec import NgramProposer
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import preset
    dev = torch.device("cuda", 0)
    cfg = preset(model)
    m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
    kw = dict(max_slots=max(batches), max_len=prompt_len + new_tokens + 16, use_graphs=True,
              max_prefill_tokens=max(batches) * prompt_len)
    off = LLMEngine(m, **kw)
    engines = {(T, w): LLMEngine(m, spec_tokens=T, proposer=Oracle(cfg.vocab_size, w), **kw)
               for T in Ts for w in (False, True)}
    for eng in engines.values():  # one set of packed weight twins (keyed by the weight) for all the runners
        eng.runner._packs = off.runner._packs
    g = torch.Generator().manual_seed(0)
    sp = SamplingParams(max_new_tokens=new_tokens, do_sample=False)
    for B in batches:
        prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g).tolist() for _ in range(B)]

        def timed(eng):
            reqs = [eng.add_request(p, sp) for p in prompts]
            eng.step()  # admit (prefill + first token) + the first decode / verify step
            torch.cuda.synchronize()
            st = eng.stats
            s0, v0, k0, t0 = st["decode_steps"], st["spec_steps"], st["decode_tokens"], time.perf_counter()
            eng.run_until_done(reqs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return {"ms_per_step": dt / max(st["decode_steps"] - s0, 1) * 1e3, "tokens_per_s": (st["decode_tokens"] - k0) / dt,
                    "verify_share": (st["spec_steps"] - v0) / max(st["decode_steps"] - s0, 1), "outs": [r.output for r in reqs]}

        base = off.generate(prompts, sp)  # warm-up + graph capture; the continuation the oracles draft
        for (T, w), eng in engines.items():
            # the script is the engine's own output: a verify step's rows take other kernels than a decode
            # step's, so a near-tie can fall the other way; iterate to the engine's own fixed point
            script = [r.output for r in base]
            for _ in range(16):
                eng.proposer.scripts = {tuple(p): o for p, o in zip(prompts, script)}
                outs = [r.output for r in eng.generate(prompts, sp)]
                if outs == script:
                    break
                script = outs
        res = {k: [] for k in [("off", False)] + list(engines)}
        for _ in range(reps):
            res[("off", False)].append(timed(off))
            for k, eng in engines.items():
                eng.proposer.seconds, eng.proposer.calls = 0.0, 0
                res[k].append(timed(eng))
        dec_ms, dec_lo, dec_hi = _stats([r["ms_per_step"] for r in res[("off", False)]], 3)
        dec_tps = _stats([r["tokens_per_s"] for r in res[("off", False)]], 1)
        ng = NgramProposer()
        toks = [p + o for p, o in zip(prompts, [r.output for r in base])]
        t0 = time.perf_counter()
        for tk in toks:
            for n in range(prompt_len + 1, len(tk), 8):
                ng.propose(tk[:n], 7)
        ngram_us = (time.perf_counter() - t0) / (len(toks) * len(range(prompt_len + 1, len(toks[0]), 8))) * 1e6
        for T in Ts:
            row = {"table": "engine", "model": model, "batch": B, "prompt_len": prompt_len, "new_tokens": new_tokens,
                   "T": T, "reps": reps, "data": "random-init weights, random prompts, scripted proposers",
                   "decode_ms_per_step": dec_ms, "decode_min": dec_lo, "decode_max": dec_hi,
                   "decode_tokens_per_s": dec_tps[0], "decode_launches_per_step": off.runner.step_launches.get(B)}
            for w, name in ((False, "right"), (True, "wrong")):
                rs = res[(T, w)]
                md, lo, hi = _stats([r["ms_per_step"] for r in rs], 3)
                eng = engines[(T, w)]
                row.update({f"{name}_ms_per_step": md, f"{name}_min": lo, f"{name}_max": hi,
                            f"{name}_tokens_per_s": _stats([r["tokens_per_s"] for r in rs], 1)[0],
                            f"{name}_verify_share": round(statistics.median(r["verify_share"] for r in rs), 3),
                            f"{name}_proposer_us_per_step": round(eng.proposer.seconds / max(eng.proposer.calls, 1) * B * 1e6, 1)})
            row["verify_launches_per_step"] = engines[(T, False)].runner.step_launches.get(
                ("spec", 1 << (B - 1).bit_length(), T))
            row["right_equals_decode_output"] = res[(T, False)][-1]["outs"] == [r.output for r in base]
            row["verify_over_decode"] = round(row["wrong_ms_per_step"] / dec_ms, 3)
            row["break_even_acceptance"] = round((row["wrong_ms_per_step"] / dec_ms - 1) / (T - 1), 3)
            row["speedup_at_acceptance_1"] = round(row["right_tokens_per_s"] / dec_tps[0], 3)
            row["speedup_at_acceptance_0"] = round(row["wrong_tokens_per_s"] / dec_tps[0], 3)
            row["ngram_proposer_us_per_call"] = round(ngram_us, 1)
            _emit(fh, row)
    del engines, off, m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "spec_decode_ab_r12.jsonl"))
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions per kernel row (>= 20)")
    ap.add_argument("--engine-reps", type=int, default=3, help="timed runs per engine and cell")
    ap.add_argument("--models", default=",".join(SHAPES))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--kvs", default="512,2048,8192")
    ap.add_argument("--Ts", default="2,4,8")
    ap.add_argument("--max-buffers", type=int, default=1024)
    ap.add_argument("--engine-models", default="gpt-j-6b,gpt-neox-20b")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=65)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spec_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    with open(a.out, "a") as fh:
        if not a.skip_kernels:
            kernel_table(fh, max(a.reps, 20), [s for s in a.models.split(",") if s], ints(a.batches), ints(a.kvs),
                         ints(a.Ts), a.max_buffers)
        if not a.skip_engine:
            for model in [s for s in a.engine_models.split(",") if s]:
                engine_table(fh, model, ints(a.batches), ints(a.Ts), a.prompt_len, a.engine_reps, a.new_tokens)


if __name__ == "__main__":
    main()
