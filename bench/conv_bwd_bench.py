#!/usr/bin/env python3
"""SD-1.5 UNet 3x3 convolution backward (channels-last bf16, N = 16) on MI355X: tuned MIOpen
(``aten.convolution_backward`` with one product in ``output_mask``) vs the native products of
ops/conv.py -- the data gradient including the weight flip (weights change every step), the weight
gradient including its split-K reduce. One JSON line per shape; every quantity is timed three times
and all three values are recorded (a shape enters ``_FAST_DGRAD`` / ``_FAST_WGRAD`` only if the slowest
native timing is below the fastest MIOpen one).

    python bench/conv_bwd_bench.py [--splits S ...]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from conv_bench import SHAPES, timeit  # (run as a script: bench/ is sys.path[0])
from kubernetes_cloud_amd.utils import miopen

UNET_SHAPES = [s for s in SHAPES if s[0] == 16]


def time3(fn):
    return [round(timeit(fn), 4) for _ in range(3)]


def rel_err(got, ref):
    return round(float((got.float() - ref).norm() / ref.norm()), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", type=int, nargs="*", default=[],
                    help="also time the weight gradient with these forced split counts (A/B of the automatic S)")
    a = ap.parse_args()
    miopen.configure()
    from kubernetes_cloud_amd.ops import _lib
    from kubernetes_cloud_amd.ops import conv as kconv
    _lib.require()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cl = torch.channels_last
    for (N, H, W, C, Co) in UNET_SHAPES:
        x = torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16).to(memory_format=cl)
        w = (torch.randn(Co, C, 3, 3, device=dev, dtype=torch.bfloat16) * 0.02).to(memory_format=cl)
        gy = torch.randn(N, Co, H, W, device=dev, dtype=torch.bfloat16).to(memory_format=cl)
        flops = 2.0 * N * H * W * Co * 9 * C
        tf = lambda ms: round(flops / min(ms) / 1e9, 1)
        rec = {"shape": [N, H, W, C, Co]}
        rec["miopen_dgrad_ms"] = time3(lambda: kconv._aten_backward(gy, x, w, (True, False, False)))
        rec["miopen_wgrad_ms"] = time3(lambda: kconv._aten_backward(gy, x, w, (False, True, False)))
        rec["miopen_dgrad_tflops"], rec["miopen_wgrad_tflops"] = tf(rec["miopen_dgrad_ms"]), tf(rec["miopen_wgrad_ms"])
        ref = kconv.conv3x3_backward_reference(gy, x, w, False, (True, True, False))
        if kconv._dgrad_native(gy, w) is not None:
            rec["native_dgrad_ms"] = time3(lambda: kconv._dgrad_native(gy, w))
            rec["native_flip_ms"] = time3(lambda: kconv.flip_weight(w))
            rec["native_dgrad_tflops"] = tf(rec["native_dgrad_ms"])
            rec["native_dgrad_rel_err"] = rel_err(kconv._dgrad_native(gy, w), ref[0])
            rec["dgrad_wins"] = max(rec["native_dgrad_ms"]) < min(rec["miopen_dgrad_ms"])
        if kconv._wgrad_native(x, gy) is not None:
            rec["wgrad_splits"] = _lib.require().kca_conv3x3_wgrad_splits(N, H, W, C, Co)
            rec["native_wgrad_ms"] = time3(lambda: kconv._wgrad_native(x, gy))
            rec["native_wgrad_tflops"] = tf(rec["native_wgrad_ms"])
            rec["native_wgrad_rel_err"] = rel_err(kconv._wgrad_native(x, gy), ref[1])
            rec["wgrad_wins"] = max(rec["native_wgrad_ms"]) < min(rec["miopen_wgrad_ms"])
            for s in a.splits:
                rec[f"native_wgrad_s{s}_ms"] = time3(lambda: kconv._wgrad_native(x, gy, s))
        rec["miopen_rel_err"] = [rel_err(g_, r_) for g_, r_ in
                                 zip(kconv._aten_backward(gy, x, w, (True, True, False))[:2], ref)]
        print(json.dumps(rec), flush=True)
        del x, w, gy, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
