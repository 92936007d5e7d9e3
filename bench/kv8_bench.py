#!/usr/bin/env python3
"""FP8 KV cache A/B (ops/kv8.py, csrc/kernels/decode_kv8.hip) against the 16-bit default.

Two tables, one JSON line per row, appended to ``--out``:

* kernel: the decode step's attention -- 16-bit ``decode_prep_attention`` (one fused launch) against
  ``kv8_prep_attention`` (prep + attention + combine launches) -- at the head shapes of GPT-J (16 x 256),
  GPT-NeoX-20B (64 x 96) and a BLOOM-176B TP=8 rank (14 x 128, ALiBi), B = 1 / 8 / 32 sequences of
  512 / 2048 / 8192 cached tokens, on paged pools (64-token pages, shuffled page ids, as the engine
  allocates them). Each repetition is one pass over enough distinct caches (>= 1 GiB of the smaller, FP8
  stream in all, four times the 256 MB Infinity Cache) that no call finds its K/V cached, replayed as
  one HIP graph (the engine replays graphs; ``--eager`` times the launches instead); the two arms
  alternate repetition by repetition; median, min and max over the repetitions as us per call and as
  GB/s of the KV bytes each arm streams (the FP8 arm's include its scales).
* engine: ms/token of ``LLMEngine`` (HIP graphs, random-init weights as bench/decode_bench.py builds
  them): the 16-bit default dispatch, ``kv_dtype="fp8"``, and ``kv_dtype`` + ``weight_dtype`` both fp8;
  all engines alive in one process on one model, timed runs alternating.

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

# local heads, KV heads, head dim, rotary dims, interleaved, ALiBi
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


def _stats(xs):
    return round(statistics.median(xs), 2), round(min(xs), 2), round(max(xs), 2)


def kernel_table(fh, reps: int, models, batches, kvs, max_buffers: int, eager: bool = False):
    from kubernetes_cloud_amd.ops import decode as dops
    from kubernetes_cloud_amd.ops import kv8
    from kubernetes_cloud_amd.ops.rope import rope_tables
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for model in models:
        s = SHAPES[model]
        H, Hkv, D, rot = s["H"], s["Hkv"], s["D"], s["rot"]
        for B in batches:
            for kv in kvs:
                nb = kv // PS
                pages = B * nb
                b8 = B * Hkv * kv * 2 * (D + 4)  # K + V bytes and scales one call streams
                b16 = B * Hkv * kv * 2 * D * 2
                nbuf = min(max_buffers, max(2, -(-ROTATE_BYTES // b8)))
                tbl = torch.randperm(pages, generator=torch.Generator().manual_seed(kv + B)).view(B, nb)
                tbl = tbl.to(torch.int32).to(dev)
                shape = (pages + 1, Hkv, PS, D)
                c16, c8 = [], []
                for _ in range(nbuf):
                    c16.append(tuple(torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16) for _ in "kv"))
                    c8.append(tuple(torch.randint(0, 0x78, shape, generator=g, device=dev, dtype=torch.uint8)
                                    for _ in "kv")
                              + tuple(torch.rand(shape[:-1], generator=g, device=dev) * 0.02 + 0.001 for _ in "kv"))
                qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g, device=dev).to(torch.bfloat16)
                cos, sin = rope_tables(rot, kv, 10000.0, dev) if rot else (None, None)
                al = (2.0 ** (-8.0 * torch.arange(1, H + 1, device=dev) / H)).float() if s["alibi"] else None
                pos = torch.full((B,), kv - 1, device=dev, dtype=torch.int32)
                lens = pos + 1
                slots = torch.arange(B, device=dev, dtype=torch.int32)
                out = torch.empty(B, H * D, device=dev, dtype=torch.bfloat16)
                n_ws = max(dops.decode_ws_floats(B, H, Hkv, D, kv), 1)
                ws16 = torch.zeros(n_ws, device=dev, dtype=torch.float32)
                ws8 = torch.zeros(n_ws, device=dev, dtype=torch.float32)
                scale = D ** -0.5

                def ref(i):
                    dops.decode_prep_attention(qkv, H, Hkv, D, rot, s["inter"], cos, sin, pos, slots, c16[i][0],
                                               c16[i][1], lens, kv, scale, al, out=out, ws=ws16, block_table=tbl)

                def new(i):
                    k, v, ks, vs = c8[i]  # (Q is re-rotated in place call after call: same work, finite values)
                    kv8.kv8_prep_attention(qkv, H, Hkv, D, rot, s["inter"], cos, sin, pos, slots, k, v, ks, vs, lens,
                                           kv, scale, al, out=out, ws=ws8, block_table=tbl)

                def as_graph(fn):  # one pass over the buffers as one HIP graph: what the engine replays
                    if eager:
                        return None
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

                def one_pass(fn, gr):
                    s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    if gr is not None:
                        gr.replay()
                    else:
                        for i in range(nbuf):
                            fn(i)
                    e0.record()
                    e0.synchronize()
                    return s0.elapsed_time(e0) / nbuf * 1e3  # us per call

                g16, g8 = as_graph(ref), as_graph(new)
                for _ in range(2):
                    one_pass(ref, g16)
                    one_pass(new, g8)
                t16, t8 = [], []
                for _ in range(reps):
                    t16.append(one_pass(ref, g16))
                    t8.append(one_pass(new, g8))
                m16, lo16, hi16 = _stats(t16)
                m8, lo8, hi8 = _stats(t8)
                _emit(fh, {"table": "kernel", "model": model, "B": B, "kv": kv, "H": H, "D": D, "page": PS,
                           "reps": reps, "timing": "eager launches" if eager else "hip graph replay", "buffers": nbuf, "rotated_MiB_fp8": round(nbuf * b8 / 2 ** 20),
                           "chunk": dops.decode_chunk(B, Hkv, kv), "bf16_us": m16, "bf16_us_min": lo16,
                           "bf16_us_max": hi16, "bf16_GBps": round(b16 / m16 / 1e3, 1), "fp8_us": m8,
                           "fp8_us_min": lo8, "fp8_us_max": hi8, "fp8_GBps": round(b8 / m8 / 1e3, 1),
                           "speedup": round(m16 / m8, 3)})
                del c16, c8, g16, g8
                torch.cuda.empty_cache()


def engine_table(fh, model: str, batches, prompt_lens, reps: int, new_tokens: int):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import preset
    dev = torch.device("cuda", 0)
    cfg = preset(model)
    m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
    # (every prompt of a cell is admitted by the first step: the timed steps are decode steps only)
    kw = dict(max_slots=max(batches), max_len=max(prompt_lens) + new_tokens + 16, use_graphs=True,
              max_prefill_tokens=max(batches) * max(prompt_lens))
    engines = {"bf16": LLMEngine(m, **kw), "kv8": LLMEngine(m, kv_dtype="fp8", **kw),
               "kv8_w8": LLMEngine(m, kv_dtype="fp8", weight_dtype="fp8", **kw)}
    assert not engines["bf16"].runner._kv8 and engines["kv8"].runner._kv8 and engines["kv8_w8"].runner._w8
    g = torch.Generator().manual_seed(0)
    sp = SamplingParams(max_new_tokens=new_tokens, do_sample=False)
    for P in prompt_lens:
        for B in batches:
            prompts = [torch.randint(0, cfg.vocab_size, (P,), generator=g).tolist() for _ in range(B)]

            def timed(eng):
                reqs = [eng.add_request(p, sp) for p in prompts]
                eng.step()  # admit (prefill + first token) + first decode
                torch.cuda.synchronize()
                s0, t0 = eng.stats["decode_steps"], time.perf_counter()
                eng.run_until_done(reqs)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / max(eng.stats["decode_steps"] - s0, 1) * 1e3

            for eng in engines.values():  # warm-up + graph capture of this bucket
                eng.generate(prompts, sp)
            ts = {k: [] for k in engines}
            for _ in range(reps):
                for k, eng in engines.items():
                    ts[k].append(timed(eng))
            row = {"table": "engine", "model": model, "batch": B, "prompt_len": P, "new_tokens": new_tokens,
                   "reps": reps, "data": "random-init weights, random prompts"}
            for k in engines:
                md, lo, hi = _stats(ts[k])
                row.update({f"{k}_ms_per_token": round(md, 3), f"{k}_min": round(lo, 3), f"{k}_max": round(hi, 3),
                            f"{k}_launches_per_step": engines[k].runner.step_launches.get(B)})
            row["kv8_speedup"] = round(row["bf16_ms_per_token"] / row["kv8_ms_per_token"], 3)
            row["kv8_w8_speedup"] = round(row["bf16_ms_per_token"] / row["kv8_w8_ms_per_token"], 3)
            row["cache_GiB"] = {k: round(e.runner.cache.nbytes() / 2 ** 30, 2) for k, e in engines.items()}
            _emit(fh, row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "kv8_decode_ab_r10.jsonl"))
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions per kernel row (>= 20)")
    ap.add_argument("--engine-reps", type=int, default=3, help="timed decode runs per engine and cell")
    ap.add_argument("--models", default=",".join(SHAPES))
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--kvs", default="512,2048,8192")
    ap.add_argument("--max-buffers", type=int, default=1024)
    ap.add_argument("--eager", action="store_true", help="time eager launches (host-bound below ~30 us per call) "
                    "instead of one HIP graph per pass")
    ap.add_argument("--engine-model", default="gpt-j-6b")
    ap.add_argument("--prompt-lens", default="512,2048")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv8_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    with open(a.out, "a") as fh:
        if not a.skip_kernels:
            kernel_table(fh, max(a.reps, 20), [s for s in a.models.split(",") if s], ints(a.batches), ints(a.kvs),
                         a.max_buffers, a.eager)
        if not a.skip_engine:
            engine_table(fh, a.engine_model, ints(a.batches), ints(a.prompt_lens), a.engine_reps, a.new_tokens)


if __name__ == "__main__":
    main()
