"""Speculative decoding (draft and verify): the decode step of T tokens per sequence.

A verify step feeds every sequence its last token and up to T - 1 drafted tokens as T consecutive rows:
row ``b * T + t`` of ``qkv`` is token ``t`` of sequence ``b`` at position ``base[b] + t``; ``n_tok[b]``
(1..T) of them are real, the rest is padding.

* ``spec_prep``            ``ops.decode.decode_prep`` row by row: RoPE on Q (in place) and K, K/V of the
                           rows ``t < n_tok[b]`` appended at ``base[b] + t``; padding rows write nothing
* ``spec_attention``       split-K attention in which the G x T queries of one (sequence, kv-head) share
                           every K/V row load: query ``t`` attends to positions
                           ``[lo, kv_lens[b] - n_tok[b] + t + 1)`` (``kv_lens``: the length after all
                           ``n_tok[b]`` tokens; ``lo`` = 0, or ``qpos + 1 - window``), ALiBi
                           ``slope * (t_key - qpos)``; padding rows come out as zeros
* ``spec_prep_attention``  the two for a verify step (``kv_lens = base + n_tok``)

bf16 / fp16 GPU tensors run ``csrc/kernels/decode_spec.hip`` (prep, attention and -- past one split --
the combine); CPU tensors run the references below, which are also the test oracle. A GPU tensor never
takes the reference path because a kernel is missing: that raises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode import _table_args, decode_chunk, decode_prep, decode_ws_floats, gather_kv

QUERIES = (2, 4, 8)  # G * T the attention kernel is instantiated for


def supported(head_dim: int, n_heads: int, kv_heads: int, T: int) -> bool:
    """Shapes ``kca_spec_attn`` takes: D % 8 == 0, D <= 256, T >= 2 and (H / Hkv) * T in {2, 4, 8}."""
    return (head_dim % 8 == 0 and 0 < head_dim <= 256 and kv_heads > 0 and n_heads % kv_heads == 0 and T >= 2
            and (n_heads // kv_heads) * T in QUERIES)


# --------------------------------------------------------------- references
@torch.no_grad()
def spec_prep_reference(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, base, n_tok, slots, T,
                        k_cache, v_cache, block_table=None):
    """``decode_prep`` on the rows ``t < n_tok[b]`` (position ``base[b] + t``); the others are left alone."""
    B = qkv.shape[0] // T
    t = torch.arange(T, device=qkv.device)[None]
    valid = (t < n_tok.long()[:, None]).reshape(-1)
    idx = valid.nonzero()[:, 0]
    if idx.numel() == 0:
        return
    pos = (base.long()[:, None] + t).reshape(-1)[idx].to(torch.int32)
    sl = slots.long()[:, None].expand(B, T).reshape(-1)[idx].to(torch.int32)
    sub = qkv[idx].contiguous()
    decode_prep(sub, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, pos, sl, k_cache, v_cache, block_table)
    qkv[idx] = sub


def spec_attention_reference(q, k_cache, v_cache, slots, kv_lens, n_tok, T, n_heads, scale, alibi=None, out=None,
                             block_table=None, window: int = 0, fp64: bool = False):
    """Row ``(b, t)``, ``t < n_tok[b]``: ``ops.decode.decode_attention_reference`` with the length
    ``kv_lens[b] - n_tok[b] + t + 1`` (fp64 arithmetic when asked); rows ``t >= n_tok[b]``: zeros."""
    B = q.shape[0] // T
    _, Hkv, _, D = k_cache.shape
    H = n_heads
    ft = torch.float64 if fp64 else torch.float32
    if out is None:
        out = torch.empty(B * T, H * D, device=q.device, dtype=q.dtype)
    for b in range(B):
        L, nt, s_ = int(kv_lens[b]), int(n_tok[b]), int(slots[b])
        kall = gather_kv(k_cache, s_, L, block_table).to(ft)
        vall = gather_kv(v_cache, s_, L, block_table).to(ft)
        for t in range(T):
            r = b * T + t
            if t >= nt:
                out[r] = 0
                continue
            n = L - nt + t + 1
            lo = max(0, n - window) if window > 0 else 0
            qb = q[r, :H * D].to(ft).view(H, D)
            kb = kall[:, lo:n].repeat_interleave(H // Hkv, 0)  # [H, n - lo, D]
            vb = vall[:, lo:n].repeat_interleave(H // Hkv, 0)
            sc = torch.einsum("hd,hnd->hn", qb, kb) * scale
            if alibi is not None:
                sc = sc + alibi.to(ft)[:, None] * (torch.arange(lo, n, device=q.device) - (n - 1)).to(ft)[None]
            out[r] = torch.einsum("hn,hnd->hd", sc.softmax(-1), vb).reshape(-1).to(out.dtype)
    return out


# ------------------------------------------------------------- dispatching
def _native(x: torch.Tensor, k_cache: torch.Tensor, *symbols: str) -> bool:
    """GPU bf16 / fp16 tensors run the kernels; a missing kernel raises (no quiet reference path)."""
    if not (x.is_cuda and k_cache.is_cuda and x.dtype in (torch.bfloat16, torch.float16)):
        return False
    assert k_cache.dtype == x.dtype, "the KV cache holds the activation's element type"
    for sym in symbols:
        if not _lib.has(sym):
            _lib.require()
            raise RuntimeError(f"{sym} missing from the kernel library (rebuild: python tools/build_ext.py)")
    return True


def _i32(*ts):
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in ts), "int32 contiguous step arrays"


def spec_prep(qkv: torch.Tensor, n_heads: int, kv_heads: int, head_dim: int, rot: int, interleaved: bool,
              cos: torch.Tensor | None, sin: torch.Tensor | None, base: torch.Tensor, n_tok: torch.Tensor,
              slots: torch.Tensor, T: int, k_cache: torch.Tensor, v_cache: torch.Tensor,
              block_table: torch.Tensor | None = None):
    """qkv [B*T, (H+2Hkv)*D] (row-strided). Rotates the Q of the rows ``t < n_tok[b]`` in place and writes
    their rotated K and V into cache[slots[b], :, base[b] + t] (paged: into its page)."""
    assert qkv.shape[0] % T == 0 and qkv.shape[0] // T == base.shape[0] == n_tok.shape[0] == slots.shape[0]
    if _native(qkv, k_cache, "kca_spec_prep"):
        assert qkv.stride(-1) == 1 and k_cache.stride(-1) == 1 and k_cache.stride() == v_cache.stride()
        _i32(base, n_tok, slots)
        tbl, tstride, shift = _table_args(block_table, k_cache)
        cap = k_cache.shape[2] if block_table is None else block_table.shape[1] * k_cache.shape[2]
        if cos is not None:
            assert cos.is_contiguous() and sin.is_contiguous() and cos.shape == sin.shape
            cap = min(cap, cos.shape[0])  # positions the rotation tables hold
        _lib.call("kca_spec_prep", qkv.data_ptr(), qkv.stride(0), qkv.shape[0] // T, T, n_heads, kv_heads, head_dim,
                  rot, int(interleaved), _lib.ptr(cos), _lib.ptr(sin), base.data_ptr(), n_tok.data_ptr(),
                  slots.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1),
                  k_cache.stride(2), tbl, tstride, shift, cap, int(qkv.dtype == torch.float16), _lib.stream())
        return
    spec_prep_reference(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, base, n_tok, slots, T,
                        k_cache, v_cache, block_table)


def spec_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor,
                   kv_lens: torch.Tensor, n_tok: torch.Tensor, T: int, n_heads: int, max_kv: int,
                   scale: float | None = None, alibi: torch.Tensor | None = None, out: torch.Tensor | None = None,
                   ws: torch.Tensor | None = None, chunk: int = 0, block_table: torch.Tensor | None = None,
                   window: int = 0) -> torch.Tensor:
    """q [B*T, >= H*D] (row-strided; e.g. the fused QKV buffer). Returns [B*T, H*D]; rows ``t >= n_tok[b]``
    are zeros. ``ws``: ``decode_ws_floats(B*T, ...)`` fp32 words; allocated here when missing or short."""
    assert q.shape[0] % T == 0
    B = q.shape[0] // T
    _, Hkv, L, D = k_cache.shape
    H = n_heads
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if _native(q, k_cache, "kca_spec_attn"):
        if out is None:  # (a shape outside ``supported`` comes back as a status: ``_lib.call`` raises)
            out = torch.empty(B * T, H * D, device=q.device, dtype=q.dtype)
        assert q.stride(-1) == 1 and out.stride(-1) == 1 and out.dtype == q.dtype and out.shape[0] == B * T
        assert k_cache.stride(-1) == 1 and k_cache.stride() == v_cache.stride()
        assert q.stride(0) % 8 == 0 and q.data_ptr() % 16 == 0, "query rows must be 16-byte aligned"
        assert slots.shape[0] == kv_lens.shape[0] == n_tok.shape[0] == B
        _i32(slots, kv_lens, n_tok)
        tbl, tstride, shift = _table_args(block_table, k_cache)
        assert 0 < max_kv <= (L if block_table is None else block_table.shape[1] * L)
        if chunk <= 0:
            chunk = decode_chunk(B, Hkv, max_kv)
        need = decode_ws_floats(B * T, H, Hkv, D, max_kv, chunk)
        if need and (ws is None or ws.numel() < need):
            ws = torch.empty(need, device=q.device, dtype=torch.float32)
        _lib.call("kca_spec_attn", q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(),
                  k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), slots.data_ptr(), kv_lens.data_ptr(),
                  n_tok.data_ptr(), out.data_ptr(), out.stride(0), _lib.ptr(ws),
                  ws.numel() if ws is not None else 0, B, T, H, Hkv, D, max_kv, chunk, float(scale),
                  _lib.ptr(alibi), tbl, tstride, shift, int(window), int(q.dtype == torch.float16), _lib.stream())
        return out
    return spec_attention_reference(q, k_cache, v_cache, slots, kv_lens, n_tok, T, H, scale, alibi, out,
                                    block_table, window)


def spec_ws_floats(B: int, T: int, H: int, Hkv: int, D: int, max_kv: int) -> int:
    """Workspace words of ``spec_attention`` with its default split (``decode_chunk`` of B sequences)."""
    return decode_ws_floats(B * T, H, Hkv, D, max_kv, decode_chunk(B, Hkv, max_kv))


def spec_prep_attention(qkv: torch.Tensor, n_heads: int, kv_heads: int, head_dim: int, rot: int, interleaved: bool,
                        cos: torch.Tensor | None, sin: torch.Tensor | None, base: torch.Tensor,
                        n_tok: torch.Tensor, slots: torch.Tensor, T: int, k_cache: torch.Tensor,
                        v_cache: torch.Tensor, kv_lens: torch.Tensor, max_kv: int, scale: float | None = None,
                        alibi: torch.Tensor | None = None, out: torch.Tensor | None = None,
                        ws: torch.Tensor | None = None, block_table: torch.Tensor | None = None,
                        window: int = 0) -> torch.Tensor:
    """``spec_prep`` + ``spec_attention`` for a verify step (``kv_lens = base + n_tok``): on the GPU the
    prep launch, the attention launch and, past one split, the combine launch."""
    spec_prep(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, base, n_tok, slots, T, k_cache, v_cache,
              block_table)
    return spec_attention(qkv, k_cache, v_cache, slots, kv_lens, n_tok, T, n_heads, max_kv, scale, alibi, out, ws,
                          block_table=block_table, window=window)


__all__ = ["spec_prep", "spec_attention", "spec_prep_attention", "spec_prep_reference", "spec_attention_reference",
           "spec_ws_floats", "supported", "QUERIES"]
