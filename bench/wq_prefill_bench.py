#!/usr/bin/env python3
"""Quantized-weight prefill A/B (ops/wq_gemm.py, csrc/kernels/gemm_wq.hip; ``prefill_weights="quantized"``).

Two tables, one JSON line per row, appended to ``--out``:

* kernel: per projection shape of GPT-J-6B and GPT-NeoX-20B, M in 128 / 512 / 2048 / 8192, FP8 and MXFP4
  weights, bf16 (plus fp16 at M = 512), three arms in one process: ``kca_wq_gemm`` (one launch, whatever
  ``wq_linear`` would dispatch: ``wq_linear_takes`` records that), the
  64-row slab loop of ``w8_linear`` / ``mx4_linear`` (what a tall input cost before), and ``F.linear``
  on the dequantized 16-bit weight (what prefill runs without the option). Each repetition is one pass
  over enough distinct weights (>= 512 MiB of the quantized stream, twice the Infinity Cache) that no
  call finds its weight cached, as in a layer loop; the arms alternate repetition by repetition; two
  warm-up passes per arm; median, min and max over the repetitions as us per call.
* engine: ``ModelRunner.prefill`` ms for prompts of 512 and 2048 tokens at batch 1 and 8 on random-init
  models, and ``torch.cuda.memory_allocated()`` of model + runner after construction, in three modes:
  16-bit, ``weight_dtype`` alone, ``weight_dtype`` + ``prefill_weights="quantized"``. The first two share
  one model, the third has a twin; the three runners are alive in one process and their timed prefills
  alternate.

Needs a GPU; reads nothing outside the repository.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

SHAPES = {"gpt-j-6b": {"qkv": (12288, 4096), "out": (4096, 4096), "fc_in": (16384, 4096), "fc_out": (4096, 16384)},
          "gpt-neox-20b": {"qkv": (18432, 6144), "out": (6144, 6144), "fc_in": (24576, 6144),
                           "fc_out": (6144, 24576)}}
ROTATE_BYTES = 512 << 20
ARMS = ("wq", "slab", "f_linear")


def _emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def _stats(xs, nd=2):
    return round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)


def kernel_table(fh, reps: int, models, ms, fmts):
    from kubernetes_cloud_amd.ops import mx4, w8
    from kubernetes_cloud_amd.ops.wq_gemm import takes_slab_loop, wq_linear
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for model in models:
        for proj, (N, K) in SHAPES[model].items():
            for fmt in fmts:
                mod, slab = (w8, w8.w8_linear) if fmt == "fp8" else (mx4, mx4.mx4_linear)
                per = N * K if fmt == "fp8" else N * K * 17 // 32
                nbuf = max(2, -(-ROTATE_BYTES // per))
                qs, wd = [], []
                for _ in range(nbuf):
                    q = mod.quantize_weight((torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16))
                    qs.append(q)
                    wd.append(mod.dequantize(q, torch.bfloat16))
                wd16 = None
                for M, dtype in [(m, torch.bfloat16) for m in ms] + ([(512, torch.float16)] if 512 in ms else []):
                    if dtype == torch.float16 and wd16 is None:
                        wd16 = [w.to(torch.float16) for w in wd]
                    ws = wd if dtype == torch.bfloat16 else wd16
                    x = (torch.randn(M, K, generator=g, device=dev) * 0.5).to(dtype)
                    y = torch.empty(M, N, device=dev, dtype=dtype)
                    fns = {"wq": (lambda i: wq_linear(x, qs[i], out=y, dispatch=False)),
                           "slab": (lambda i: slab(x, qs[i], out=y)), "f_linear": (lambda i: F.linear(x, ws[i]))}

                    def one_pass(fn):
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for i in range(nbuf):
                            fn(i)
                        e.record()
                        e.synchronize()
                        return s.elapsed_time(e) / nbuf * 1e3  # us per call

                    n = reps if M <= 512 else max(reps // 2, 10)
                    for _ in range(2):  # warm-up: code objects, hipBLASLt's choice
                        for a in ARMS:
                            one_pass(fns[a])
                    ts = {a: [] for a in ARMS}
                    for _ in range(n):
                        for a in ARMS:
                            ts[a].append(one_pass(fns[a]))
                    row = {"table": "kernel", "model": model, "proj": proj, "fmt": fmt,
                           "dtype": str(dtype).replace("torch.", ""), "M": M, "N": N, "K": K, "reps": n, "buffers": nbuf}
                    for a in ARMS:
                        med, lo, hi = _stats(ts[a])
                        row.update({f"{a}_us": med, f"{a}_us_min": lo, f"{a}_us_max": hi})
                    row["wq_TFLOPs"] = round(2.0 * M * N * K / row["wq_us"] / 1e6, 1)
                    row["slab_over_wq"] = round(row["slab_us"] / row["wq_us"], 3)
                    row["wq_over_f_linear"] = round(row["wq_us"] / row["f_linear_us"], 3)
                    # outside run-to-run spread: the slowest wq pass against the fastest slab pass
                    row["wq_beats_slab_outside_spread"] = row["wq_us_max"] < row["slab_us_min"]
                    row["wq_linear_takes"] = "slab" if takes_slab_loop(M, N, K, 0 if fmt == "fp8" else 1) else "wq"
                    _emit(fh, row)
                del qs, wd, wd16
                gc.collect()
                torch.cuda.empty_cache()


def engine_table(fh, models, fmts, cases, reps: int):
    from kubernetes_cloud_amd.engine.runner import ModelRunner
    from kubernetes_cloud_amd.models.causal_lm import build_model
    from kubernetes_cloud_amd.models.config import preset
    dev = torch.device("cuda", 0)
    max_b, max_t = max(b for b, _ in cases), max(t for _, t in cases)
    kw = dict(max_slots=max_b, max_len=max_t + 16, use_graphs=False)

    def alloc():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    for model in models:
        cfg = preset(model)
        a0 = alloc()
        m16 = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
        model_bytes = alloc() - a0
        r16 = ModelRunner(m16, **kw)
        mem16 = alloc() - a0
        for fmt in fmts:
            a1 = alloc()
            rq = ModelRunner(m16, weight_dtype=fmt, **kw)
            mem_q = model_bytes + alloc() - a1  # the shared model plus everything this runner allocated
            a2 = alloc()
            mp = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0).eval()
            rp = ModelRunner(mp, weight_dtype=fmt, prefill_weights="quantized", **kw)
            mem_p = alloc() - a2
            wb = rp.weight_bytes()
            runners = {"16bit": r16, "weights": rq, "weights+prefill": rp}
            g = torch.Generator().manual_seed(0)
            for B, T in cases:
                ids = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(dev)
                slots = list(range(B))

                def timed(r):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    r.prefill(ids, slots)
                    e.record()
                    e.synchronize()
                    return s.elapsed_time(e)

                for r in runners.values():
                    timed(r)
                n = reps if B * T <= 4096 else max(reps // 2, 3)
                ts = {k: [] for k in runners}
                for _ in range(n):
                    for k, r in runners.items():
                        ts[k].append(timed(r))
                row = {"table": "engine", "model": model, "fmt": fmt, "batch": B, "prompt_len": T, "reps": n,
                       "data": "random-init weights, random prompts"}
                for k in runners:
                    med, lo, hi = _stats(ts[k], 3)
                    row.update({f"{k}_prefill_ms": med, f"{k}_min": lo, f"{k}_max": hi})
                row["weights+prefill_over_16bit"] = round(row["weights+prefill_prefill_ms"] / row["16bit_prefill_ms"], 3)
                row["wq_prefill_steps"] = rp.wq_prefill_steps
                _emit(fh, row)
            _emit(fh, {"table": "memory", "model": model, "fmt": fmt, "max_slots": max_b, "max_len": max_t + 16,
                       "allocated_16bit": mem16, "allocated_weights": mem_q, "allocated_weights+prefill": mem_p,
                       "saved_vs_16bit": mem16 - mem_p, "released_minus_quantized": wb["released_16bit"] - wb["quantized"],
                       **{f"weight_bytes_{k}": v for k, v in wb.items()}, "kv_cache_bytes": rp.cache.nbytes()})
            del rq, rp, mp, runners
            gc.collect()
            torch.cuda.empty_cache()
        del r16, m16
        gc.collect()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "wq_prefill_ab_r13.jsonl"))
    ap.add_argument("--reps", type=int, default=20,
                    help="timed repetitions per kernel row (half of it, >= 10, above M = 512)")
    ap.add_argument("--engine-reps", type=int, default=5)
    ap.add_argument("--models", default="gpt-j-6b,gpt-neox-20b")
    ap.add_argument("--ms", default="128,512,2048,8192")
    ap.add_argument("--fmts", default="fp8,mxfp4")
    ap.add_argument("--cases", default="1x512,1x2048,8x512,8x2048", help="engine table: batch x prompt length")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wq_prefill_bench: no GPU (timings are taken on the device or not at all)")
    from kubernetes_cloud_amd.ops import _lib
    _lib.require()
    models = [s for s in a.models.split(",") if s]
    fmts = [s for s in a.fmts.split(",") if s]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        if not a.skip_kernels:
            kernel_table(fh, max(a.reps, 20), models, [int(m) for m in a.ms.split(",")], fmts)
        if not a.skip_engine:
            engine_table(fh, models, fmts, [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")],
                         a.engine_reps)


if __name__ == "__main__":
    main()
