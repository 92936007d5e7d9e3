#!/usr/bin/env python3
"""MXFP4 weight-only decode A/B (ops/mx4.py, csrc/kernels/gemv_mx4.hip) against the FP8 weight option
and the 16-bit default.

Two tables, one JSON line per row, appended to ``--out``:

* kernel: three arms on the GPT-J, NeoX-20B and BLOOM-TP8-rank projection shapes at M = 1, 8, 32 --
  the bf16 path the runner dispatches today for the same (M, N, K) (``skinny_linear`` at M = 1, the
  matrix-core ``skinny_mm.mm`` on the packed weight twin up to the layer kind's batch cap, ``F.linear``
  above it), ``kca_w8_gemm`` and ``kca_mx4_gemm``. Each repetition is one pass over enough distinct
  weight buffers (>= 1 GiB of the smallest stream, the MXFP4 one: four times the 256 MB Infinity Cache)
  that no call finds its weight cached; the arms alternate repetition by repetition; median, min and
  max over the repetitions as us per call and as effective GB/s of the weight bytes each arm streams
  (2, 1 and 17/32 bytes per weight).
* decode: ms/token of ``LLMEngine`` (HIP graphs, random-init weights as bench/decode_bench.py builds
  them) with 16-bit, ``weight_dtype="fp8"`` and ``weight_dtype="mxfp4"`` weights, the three engines
  alive in one process on one model, timed runs alternating.

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

from w8_bench import MODELS, ROTATE_BYTES  # the same projection shapes and rotation size

ARMS = ("bf16", "fp8", "mxfp4")


def _emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def _stats(xs, nd=2):
    return round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)


def kernel_table(fh, reps: int, ms=(1, 8, 32), models=None):
    from kubernetes_cloud_amd.ops import mx4, w8
    from kubernetes_cloud_amd.ops import skinny_mm as smm
    from kubernetes_cloud_amd.ops.gemv import skinny_linear
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for model, spec in MODELS.items():
        if models and model not in models:
            continue
        for proj, (N, K) in spec["shapes"].items():
            nbuf = max(4, -(-ROTATE_BYTES // (N * K * 17 // 32)))  # sized by the smallest (MXFP4) stream
            ws = [(torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(nbuf)]
            q8 = [w8.quantize_weight(w) for w in ws]
            q4 = [mx4.quantize_weight(w) for w in ws]
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
                fns = {"bf16": ref, "fp8": (lambda i: w8.w8_linear(x, q8[i], out=y)),
                       "mxfp4": (lambda i: mx4.mx4_linear(x, q4[i], out=y))}

                def one_pass(fn):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for i in range(nbuf):
                        fn(i)
                    e.record()
                    e.synchronize()
                    return s.elapsed_time(e) / nbuf * 1e3  # us per call

                for _ in range(2):  # warm-up: code objects, hipBLASLt's choice
                    for a in ARMS:
                        one_pass(fns[a])
                ts = {a: [] for a in ARMS}
                for _ in range(reps):
                    for a in ARMS:
                        ts[a].append(one_pass(fns[a]))
                row = {"table": "kernel", "model": model, "proj": proj, "M": M, "N": N, "K": K, "reps": reps,
                       "buffers": nbuf, "bf16_path": path}
                bytes_per = {"bf16": N * K * 2, "fp8": N * K + 4 * N, "mxfp4": N * K // 2 + N * K // 32}
                for a in ARMS:
                    med, lo, hi = _stats(ts[a])
                    row.update({f"{a}_us": med, f"{a}_us_min": lo, f"{a}_us_max": hi,
                                f"{a}_GBps": round(bytes_per[a] / med / 1e3, 1)})
                row["mxfp4_vs_bf16"] = round(row["bf16_us"] / row["mxfp4_us"], 3)
                row["mxfp4_vs_fp8"] = round(row["fp8_us"] / row["mxfp4_us"], 3)
                _emit(fh, row)
            del ws, q8, q4, packs
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
        engines = {"bf16": LLMEngine(m, **kw), "fp8": LLMEngine(m, weight_dtype="fp8", **kw),
                   "mxfp4": LLMEngine(m, weight_dtype="mxfp4", **kw)}
        assert engines["bf16"].runner._w8 is None and engines["bf16"].runner._mx4 is None
        assert engines["fp8"].runner._w8 is not None and engines["mxfp4"].runner._mx4 is not None
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
            row = {"table": "decode", "model": model, "batch": B, "prompt_len": prompt_len, "new_tokens": new_tokens,
                   "reps": reps}
            for a in ARMS:
                med, lo, hi = _stats(ts[a], 3)
                row.update({f"{a}_ms_per_token": med, f"{a}_min": lo, f"{a}_max": hi,
                            f"{a}_launches_per_step": engines[a].runner.step_launches.get(B)})
            r4 = engines["mxfp4"].runner
            row.update({"mxfp4_vs_bf16": round(row["bf16_ms_per_token"] / row["mxfp4_ms_per_token"], 3),
                        "mxfp4_vs_fp8": round(row["fp8_ms_per_token"] / row["mxfp4_ms_per_token"], 3),
                        "mxfp4_mx4_steps": r4.mx4_steps, "mxfp4_other_steps": r4.w8_steps + r4.fused_steps + r4.batched_steps,
                        "data": "random-init weights, random prompts"})
            _emit(fh, row)
        del engines, m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mx4_decode_ab_r11.jsonl"))
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions per kernel row (>= 20)")
    ap.add_argument("--decode-reps", type=int, default=3, help="timed decode runs per engine and batch")
    ap.add_argument("--models", default="gpt-j-6b,gpt-neox-20b")
    ap.add_argument("--kernel-models", default="", help="comma list of kernel-table models (default: all)")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx4_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        if not a.skip_kernels:
            kernel_table(fh, max(a.reps, 20), models=[s for s in a.kernel_models.split(",") if s])
        if not a.skip_decode:
            decode_table(fh, [s for s in a.models.split(",") if s], [int(b) for b in a.batches.split(",")],
                         a.decode_reps, a.prompt_len, a.new_tokens)


if __name__ == "__main__":
    main()
