#!/usr/bin/env python3
"""FP8 weight-only decode A/B (ops/w8.py, csrc/kernels/gemv_w8.hip) against the 16-bit default.

Two tables, one JSON line per row, appended to ``--out``:

* kernel: ``kca_w8_gemm`` against the bf16 path the runner dispatches today for the same (M, N, K) --
  ``skinny_linear`` at M = 1, the matrix-core ``skinny_mm.mm`` on the packed weight twin up to the layer
  kind's batch cap, ``F.linear`` (hipBLASLt) above it -- on the GPT-J, NeoX-20B and BLOOM-TP8-rank
  projection shapes at M = 1, 8, 32. Each repetition is one pass over enough distinct weight buffers
  (>= 1 GiB in all, four times the 256 MB Infinity Cache) that no call finds its weight cached; the two
  arms alternate repetition by repetition; median, min and max over the repetitions as us per call and
  as effective GB/s of the weight bytes each arm streams.
* decode: ms/token of ``LLMEngine`` (HIP graphs, random-init weights as bench/decode_bench.py builds
  them) with and without ``weight_dtype="fp8"``, both engines alive in one process on one model, timed
  runs alternating.

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
import torch.nn.functional as F

# (N, K) of the four projections; cap: largest batch the 16-bit runner gives the matrix-core layer
MODELS = {
    "gpt-j-6b": dict(cap=16, shapes={"qkv": (12288, 4096), "out": (4096, 4096), "fc_in": (16384, 4096),
                                     "fc_out": (4096, 16384)}),
    "gpt-neox-20b": dict(cap=64, shapes={"qkv": (18432, 6144), "out": (6144, 6144), "fc_in": (24576, 6144),
                                         "fc_out": (6144, 24576)}),
    "bloom-176b-tp8-rank": dict(cap=16, shapes={"qkv": (5376, 14336), "out": (14336, 1792), "fc_in": (7168, 14336),
                                                "fc_out": (14336, 7168)}),
}
ROTATE_BYTES = 1 << 30


def _emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def _stats(xs):
    return round(statistics.median(xs), 2), round(min(xs), 2), round(max(xs), 2)


def kernel_table(fh, reps: int, ms=(1, 8, 32)):
    from kubernetes_cloud_amd.ops import skinny_mm as smm
    from kubernetes_cloud_amd.ops import w8
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for model, spec in MODELS.items():
        for proj, (N, K) in spec["shapes"].items():
            nbuf = max(4, -(-ROTATE_BYTES // (N * K)))  # sized by the smaller (FP8) stream
            ws = [(torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(nbuf)]
            qs = [w8.quantize_weight(w) for w in ws]
            packs = [smm.pack_weight(w) for w in ws] if smm.PACK else [None] * nbuf
            for M in ms:
                x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                if M == 1:
                    path, ref = "skinny_linear", (lambda i: skinny_linear(x, ws[i], out=y))
                elif M <= spec["cap"]:
                    path, ref = "skinny_mm.mm", (lambda i: smm.mm(x, ws[i], out=y, packed=packs[i]))
                else:
                    path, ref = "F.linear", (lambda i: F.linear(x, ws[i]))
                new = lambda i: w8.w8_linear(x, qs[i], out=y)  # noqa: E731

                def one_pass(fn):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for i in range(nbuf):
                        fn(i)
                    e.record()
                    e.synchronize()
                    return s.elapsed_time(e) / nbuf * 1e3  # us per call

                for _ in range(2):  # warm-up: code objects, hipBLASLt's choice
                    one_pass(ref)
                    one_pass(new)
                t16, t8 = [], []
                for _ in range(reps):
                    t16.append(one_pass(ref))
                    t8.append(one_pass(new))
                m16, lo16, hi16 = _stats(t16)
                m8, lo8, hi8 = _stats(t8)
                _emit(fh, {"table": "kernel", "model": model, "proj": proj, "M": M, "N": N, "K": K, "reps": reps,
                           "buffers": nbuf, "bf16_path": path, "bf16_us": m16, "bf16_us_min": lo16,
                           "bf16_us_max": hi16, "bf16_GBps": round(N * K * 2 / m16 / 1e3, 1), "fp8_us": m8,
                           "fp8_us_min": lo8, "fp8_us_max": hi8, "fp8_GBps": round(N * K / m8 / 1e3, 1),
                           "speedup": round(m16 / m8, 3)})
            del ws, qs, packs
            torch.cuda.empty_cache()


def decode_table(fh, models, batches, reps: int, prompt_len: int, new_tokens: int):
    from kubernetes_cloud_amd.engine.llm_engine import LLMEngine, SamplingParams
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import preset
    dev = torch.device("cuda", 0)
    for model in models:
        cfg = preset(model)
        m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
        kw = dict(max_slots=max(batches), max_len=prompt_len + new_tokens + 16, use_graphs=True)
        engines = {"bf16": LLMEngine(m, **kw), "fp8": LLMEngine(m, weight_dtype="fp8", **kw)}
        assert engines["bf16"].runner._w8 is None and engines["fp8"].runner._w8 is not None
        g = torch.Generator().manual_seed(0)
        sp = SamplingParams(max_new_tokens=new_tokens, do_sample=False)
        for B in batches:
            prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g).tolist() for _ in range(B)]

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
            m16, lo16, hi16 = _stats(ts["bf16"])
            m8, lo8, hi8 = _stats(ts["fp8"])
            r8 = engines["fp8"].runner
            _emit(fh, {"table": "decode", "model": model, "batch": B, "prompt_len": prompt_len,
                       "new_tokens": new_tokens, "reps": reps, "bf16_ms_per_token": round(m16, 3),
                       "bf16_min": round(lo16, 3), "bf16_max": round(hi16, 3), "fp8_ms_per_token": round(m8, 3),
                       "fp8_min": round(lo8, 3), "fp8_max": round(hi8, 3), "speedup": round(m16 / m8, 3),
                       "fp8_w8_steps": r8.w8_steps, "fp8_launches_per_step": r8.step_launches.get(B),
                       "bf16_launches_per_step": engines["bf16"].runner.step_launches.get(B),
                       "data": "random-init weights, random prompts"})
        del engines, m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "w8_decode_ab_r9.jsonl"))
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions per kernel row (>= 20)")
    ap.add_argument("--decode-reps", type=int, default=3, help="timed decode runs per engine and batch")
    ap.add_argument("--models", default="gpt-j-6b,gpt-neox-20b")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("w8_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        if not a.skip_kernels:
            kernel_table(fh, max(a.reps, 20))
        if not a.skip_decode:
            decode_table(fh, [s for s in a.models.split(",") if s], [int(b) for b in a.batches.split(",")],
                         a.decode_reps, a.prompt_len, a.new_tokens)


if __name__ == "__main__":
    main()
