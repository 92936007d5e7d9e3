"""Prefill attention over the KV cache: the queries of a prompt chunk read their keys through the block table.

Row ``r`` of a launch holds ``lens[r]`` queries (padded to ``T``); query ``i`` sits at position
``start[r] + i`` and attends keys ``0 .. start[r] + i`` of slot ``slots[r]``. Every key -- the chunk's own
included, which ``KVCache.write`` stored just before -- is read from the cache, so the same call serves a
prefix-cache hit (``start`` = the adopted prefix), a chunk of ``prefill_chunk`` and a fresh prompt in a mixed
batch (``start`` = 0). ALiBi is ``slope * (key_pos - query_pos)``; queries ``i >= lens[r]`` come out as zeros.

* ``prefill_paged_attention``            bf16 / fp16 GPU tensors run ``csrc/kernels/prefill_paged.hip``: one
                                         launch for the whole batch, no workspace, no atomics
* ``prefill_paged_attention_reference``  the same in torch over ``ops.decode.gather_kv``: the CPU path and
                                         the test oracle
* ``supported``                          the shapes the kernel takes

A GPU tensor never takes the reference path because a kernel is missing: that raises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode import _table_args, gather_kv


def supported(head_dim: int, n_heads: int, kv_heads: int, window: int = 0) -> bool:
    """Shapes ``kca_prefill_paged_attn`` takes: D % 8 == 0, D <= 256 (padded to a compiled head dim as in
    ``attention.hip``), H % Hkv == 0 and no sliding window."""
    return (head_dim % 8 == 0 and 0 < head_dim <= 256 and kv_heads > 0 and n_heads % kv_heads == 0
            and window == 0)


def prefill_paged_attention_reference(q, k_cache, v_cache, slots, start, lens, scale=None, alibi=None, out=None,
                                      block_table=None, fp64: bool = False):
    """q [n, T, H, D] -> [n, T, H, D] in fp32 arithmetic (fp64 when asked): per row a softmax over the
    gathered keys ``[0, start + i]``; queries ``i >= lens[r]`` are zeros."""
    n, T, H, D = q.shape
    Hkv = k_cache.shape[1]
    ft = torch.float64 if fp64 else torch.float32
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty(n, T, H, D, device=q.device, dtype=q.dtype)
    for r in range(n):
        s0, ln, sl = int(start[r]), min(int(lens[r]), T), int(slots[r])
        out[r, ln:] = 0
        if ln <= 0:
            continue
        L = s0 + ln
        kall = gather_kv(k_cache, sl, L, block_table).to(ft).repeat_interleave(H // Hkv, 0)  # [H, L, D]
        vall = gather_kv(v_cache, sl, L, block_table).to(ft).repeat_interleave(H // Hkv, 0)
        sc = torch.einsum("thd,hld->htl", q[r, :ln].to(ft), kall) * scale
        qpos = s0 + torch.arange(ln, device=q.device)[:, None]
        kpos = torch.arange(L, device=q.device)[None, :]
        if alibi is not None:
            sc = sc + alibi.to(ft).view(H, 1, 1) * (kpos - qpos).to(ft)
        sc = sc.masked_fill(kpos > qpos, float("-inf"))
        out[r, :ln] = torch.einsum("htl,hld->thd", sc.softmax(-1), vall).to(out.dtype)
    return out


def _native(x: torch.Tensor, k_cache: torch.Tensor, symbol: str) -> bool:
    """GPU bf16 / fp16 tensors run the kernel; a missing kernel raises (no quiet reference path)."""
    if not (x.is_cuda and k_cache.is_cuda and x.dtype in (torch.bfloat16, torch.float16)):
        return False
    assert k_cache.dtype == x.dtype, "the KV cache holds the activation's element type"
    if not _lib.has(symbol):
        _lib.require()
        raise RuntimeError(f"{symbol} missing from the kernel library (rebuild: python tools/build_ext.py)")
    return True


def prefill_paged_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor,
                            start: torch.Tensor, lens: torch.Tensor, scale: float | None = None,
                            alibi: torch.Tensor | None = None, out: torch.Tensor | None = None,
                            block_table: torch.Tensor | None = None) -> torch.Tensor:
    """q [n, T, H, D] (any row / token / head strides, e.g. a view of the fused QKV output); k_cache / v_cache
    the layer's 16-bit caches, paged ``[pages + 1, Hkv, PS, D]`` with ``block_table`` or contiguous
    ``[slots + 1, Hkv, max_len, D]``; ``slots`` / ``start`` / ``lens`` int32 [n]. Returns [n, T, H, D]."""
    n, T, H, D = q.shape
    Hkv = k_cache.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    assert slots.shape[0] == start.shape[0] == lens.shape[0] == n
    if _native(q, k_cache, "kca_prefill_paged_attn"):
        if out is None:  # (a shape outside ``supported`` comes back as a status: ``_lib.call`` raises)
            out = torch.empty(n, T, H, D, device=q.device, dtype=q.dtype)
        assert out.shape == q.shape and out.dtype == q.dtype and q.stride(-1) == 1 and out.stride(-1) == 1
        assert k_cache.shape[3] == D and k_cache.stride(-1) == 1 and k_cache.stride() == v_cache.stride()
        assert all(t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda for t in (slots, start, lens)), \
            "int32 contiguous step arrays on the device"
        if alibi is not None:
            assert alibi.dtype == torch.float32 and alibi.is_contiguous() and alibi.numel() == H
        tbl, tstride, shift = _table_args(block_table, k_cache)
        n_slots = k_cache.shape[0] if block_table is None else block_table.shape[0]
        cap = k_cache.shape[2] if block_table is None else block_table.shape[1] * k_cache.shape[2]
        _lib.call("kca_prefill_paged_attn", q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), out.data_ptr(),
                  out.stride(0), out.stride(1), out.stride(2), k_cache.data_ptr(), v_cache.data_ptr(),
                  k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), slots.data_ptr(), start.data_ptr(),
                  lens.data_ptr(), n, T, H, Hkv, D, float(scale), _lib.ptr(alibi), tbl, tstride, shift, n_slots,
                  k_cache.shape[0], cap, int(q.dtype == torch.float16), _lib.stream())
        return out
    return prefill_paged_attention_reference(q, k_cache, v_cache, slots, start, lens, scale, alibi, out, block_table)


__all__ = ["prefill_paged_attention", "prefill_paged_attention_reference", "supported"]
