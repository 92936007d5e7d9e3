#!/usr/bin/env python3
"""Prefix caching A/B (ops/prefill_paged.py, csrc/kernels/prefill_paged.hip, the prefix index of KVCache).

Two tables, one JSON line per row, appended to ``--out``; one process, the arms alternating repetition by
repetition after warm-up, device events, median (min..max):

* attention: the continued-prefill attention of one layer, two arms --
    gather  ``ModelRunner._continued_attention``: per row, the slot's K and V gathered out of the pages into
            fresh tensors and ``ops.flash_attention`` on that row (what runs without ``prefix_cache``);
    paged   ``ops.prefill_paged.prefill_paged_attention``: one launch for the batch, keys read through the
            block table --
  at the head shapes of GPT-J (16 x 256) and GPT-NeoX-20B (64 x 96), 1 / 8 / 32 rows, a cached prefix of
  512 / 2048 tokens and a suffix of 64 / 512 tokens, pages of 64.
* engine: ``LLMEngine`` on random-init weights, 32 requests that share a 1024-token prefix and end in 64
  tokens of their own, arriving together after one request that carried the prefix: time to the first
  token (arrival to the first sampled token, per request) and the wall time of the admission step, with
  ``prefix_cache`` on against off on the same model.

Needs a GPU; reads nothing outside the repository.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = {"gpt-j-6b": dict(H=16, D=256), "gpt-neox-20b": dict(H=64, D=96)}
PS = 64


def _emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def _stats(xs, nd=3):
    return round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)


def attention_table(fh, reps: int, models, rows_list, prefixes, suffixes):
    from kubernetes_cloud_amd.engine.runner import KVCache, ModelRunner
    from kubernetes_cloud_amd.ops import prefill_paged as pp
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for model in models:
        H, D = SHAPES[model]["H"], SHAPES[model]["D"]
        at = types.SimpleNamespace(window=0, scale=D ** -0.5, alibi=None)
        for n in rows_list:
            for prefix in prefixes:
                for suffix in suffixes:
                    kv = prefix + suffix
                    cache = KVCache(1, n, H, kv, D, dev, torch.bfloat16, page_size=PS)
                    order = torch.randperm(n * cache.blocks, generator=torch.Generator().manual_seed(kv + n)).tolist()
                    cache.free_pages = order  # shuffled pages, as a cache that has served for a while
                    for s_ in range(n):
                        cache.reserve(s_, kv)
                    cache.sync()
                    cache.k[0].normal_(generator=g)
                    cache.v[0].normal_(generator=g)
                    stub = types.SimpleNamespace(cache=cache, _kv8=False, layer_devs=[dev])
                    qkv = torch.randn(n, suffix, 3, H, D, generator=g, device=dev).to(torch.bfloat16)
                    q = qkv[:, :, 0]
                    slots, lens, start = list(range(n)), [suffix] * n, [prefix] * n
                    rows_d = torch.tensor([slots, start, lens], dtype=torch.int32, device=dev)
                    out = torch.empty(n, suffix, H, D, device=dev, dtype=torch.bfloat16)

                    def arm_gather():
                        return ModelRunner._continued_attention(stub, 0, q, slots, lens, start, at)

                    def arm_paged():
                        return pp.prefill_paged_attention(q, cache.k[0], cache.v[0], rows_d[0], rows_d[1], rows_d[2],
                                                          at.scale, None, out=out, block_table=cache.table)

                    def timed(fn):
                        s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s0.record()
                        fn()
                        e0.record()
                        e0.synchronize()
                        return s0.elapsed_time(e0)

                    arms = {"gather": arm_gather, "paged": arm_paged}
                    diff = (arm_gather().float() - arm_paged().float()).abs().max().item()
                    for _ in range(2):
                        for fn in arms.values():
                            timed(fn)
                    ts = {k: [] for k in arms}
                    for _ in range(reps):
                        for k, fn in arms.items():
                            ts[k].append(timed(fn))
                    row = {"table": "attention", "model": model, "H": H, "D": D, "rows": n, "prefix": prefix,
                           "suffix": suffix, "page": PS, "reps": reps, "timing": "device events, eager launches",
                           "max_abs_diff": round(diff, 5)}
                    for k in arms:
                        md, lo, hi = _stats(ts[k])
                        row.update({f"{k}_ms": md, f"{k}_ms_min": lo, f"{k}_ms_max": hi})
                    row["gather_over_paged"] = round(row["gather_ms"] / row["paged_ms"], 2)
                    # slower by more than the repeat-to-repeat spread: the paged arm's best run behind the
                    # gather arm's worst
                    row["paged_slower"] = bool(row["paged_ms_min"] > row["gather_ms_max"])
                    _emit(fh, row)
                    del cache, stub, qkv, q, out
                    torch.cuda.empty_cache()


def engine_table(fh, model: str, n_req: int, prefix_len: int, tail_len: int, reps: int):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import preset
    dev = torch.device("cuda", 0)
    cfg = preset(model)
    m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
    L = prefix_len + tail_len
    kw = dict(max_slots=n_req, max_len=L + 16, use_graphs=True, max_prefill_tokens=n_req * L)
    engines = {"off": LLMEngine(m, **kw), "on": LLMEngine(m, prefix_cache=True, **kw)}
    engines["on"].runner._packs = engines["off"].runner._packs
    g = torch.Generator().manual_seed(0)
    prefix = torch.randint(0, cfg.vocab_size, (prefix_len,), generator=g).tolist()
    tails = [torch.randint(0, cfg.vocab_size, (tail_len,), generator=g).tolist() for _ in range(n_req + 1)]
    sp = SamplingParams(max_new_tokens=1, do_sample=False)

    def timed(eng):
        st0 = dict(eng.stats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reqs = [eng.add_request(prefix + t, sp) for t in tails[1:]]
        eng.run_until_done(reqs)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ttft = [(r.t_first - r.t_arrive) * 1e3 for r in reqs]
        return {"wall_ms": wall, "ttft_ms": statistics.median(ttft), "ttft_max_ms": max(ttft),
                "prefill_tokens": eng.stats["prefill_tokens"] - st0["prefill_tokens"],
                "hit_tokens": eng.stats.get("prefix_hit_tokens", 0) - st0.get("prefix_hit_tokens", 0),
                "outs": [r.output for r in reqs]}

    for eng in engines.values():  # the request that carries the prefix (and the warm-up of both arms)
        eng.generate([prefix + tails[0]], sp)
        timed(eng)
    res = {k: [] for k in engines}
    for _ in range(reps):
        for k, eng in engines.items():
            res[k].append(timed(eng))
    row = {"table": "engine", "model": model, "requests": n_req, "prefix": prefix_len, "tail": tail_len,
           "reps": reps, "page": engines["on"].runner.cache.page_size,
           "data": "random-init weights, random tokens; max_new_tokens=1, one admission step",
           "same_first_tokens": res["on"][-1]["outs"] == res["off"][-1]["outs"],
           "paged_prefill_calls": engines["on"].runner.paged_prefill_calls,
           "gather_prefill_calls": engines["on"].runner.gather_prefill_calls}
    for k in engines:
        for f in ("wall_ms", "ttft_ms", "ttft_max_ms"):
            md, lo, hi = _stats([r[f] for r in res[k]], 2)
            row.update({f"{k}_{f}": md, f"{k}_{f}_min": lo, f"{k}_{f}_max": hi})
        row[f"{k}_prefill_tokens"] = res[k][-1]["prefill_tokens"]
        row[f"{k}_hit_tokens"] = res[k][-1]["hit_tokens"]
    row["ttft_off_over_on"] = round(row["off_ttft_ms"] / row["on_ttft_ms"], 2)
    row["prefill_ms_off_over_on"] = round(row["off_wall_ms"] / row["on_wall_ms"], 2)
    _emit(fh, row)
    del engines, m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "prefix_cache_ab_r14.jsonl"))
    ap.add_argument("--reps", type=int, default=10, help="timed repetitions per attention row and arm")
    ap.add_argument("--engine-reps", type=int, default=3, help="timed runs per engine arm")
    ap.add_argument("--models", default=",".join(SHAPES))
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--prefixes", default="512,2048")
    ap.add_argument("--suffixes", default="64,512")
    ap.add_argument("--engine-models", default="gpt-j-6b")
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--prefix-len", type=int, default=1024)
    ap.add_argument("--tail-len", type=int, default=64)
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prefix_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    with open(a.out, "a") as fh:
        if not a.skip_attention:
            attention_table(fh, a.reps, [s for s in a.models.split(",") if s], ints(a.rows), ints(a.prefixes),
                            ints(a.suffixes))
        if not a.skip_engine:
            for model in [s for s in a.engine_models.split(",") if s]:
                engine_table(fh, model, a.requests, a.prefix_len, a.tail_len, a.engine_reps)


if __name__ == "__main__":
    main()
