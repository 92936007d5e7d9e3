"""FP8 KV cache for decode: e4m3 K/V rows with one fp32 scale per (token, kv-head) row.

A cache row -- the D values of one (token, kv-head) -- is stored as D OCP ``e4m3fn`` bytes plus one
fp32 scale, by ``ops.w8.quantize_weight``'s rule along the last dimension (``quantize_rows``): scale =
absmax / 448 (1 for an all-zero row), the fp32 quotient clamped to +-448 and rounded to nearest even,
non-finite inputs counted as 0 (so 0x7F / 0xFF never appear). (D + 4) / 2D of the 16-bit cache's bytes:
0.53 / 0.52 / 0.52 / 0.51 at D = 64 / 96 / 128 / 256.

Caches keep ``ops.decode``'s layout with one byte per element -- ``k_cache`` / ``v_cache``
[slots, Hkv, max_len, D] uint8 (paged: pools [pages, Hkv, PS, D]) -- plus ``k_scale`` / ``v_scale`` of
shape ``cache.shape[:-1]`` fp32, addressed through the same block table.

* ``kv8_prep``            RoPE on the step's Q (in place) and K; the rotated K is rounded to the
                          activation's type first (the row the 16-bit cache would hold), then K and V
                          rows are quantized and appended
* ``kv8_attention``       split-K decode attention over the byte cache:
                          score(t) = scale * k_scale[t] * sum_d q[d] k8[t, d] + ALiBi,
                          out = sum_t p[t] v_scale[t] v8[t, :] / sum_t p[t]; fp32 accumulation, one
                          rounding to the output type; the row scales multiply fp32 sums, never the bytes
* ``kv8_prep_attention``  the two for a decode step (kv_lens = pos + 1)

bf16 / fp16 GPU tensors run ``csrc/kernels/decode_kv8.hip`` (prep, attention and -- past one split --
the combine: two or three launches per layer); CPU tensors run the references below. A GPU tensor
never takes the reference path because a kernel is missing: that raises.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode import (_prep_rows_reference, _table_args, decode_chunk, decode_ws_floats, gather_kv)
from .w8 import quantize_weight

GROUPS = (1, 2, 4, 8)  # GQA group sizes the attention kernel is instantiated for


def supported(head_dim: int, n_heads: int, kv_heads: int) -> bool:
    """Head shapes ``kca_kv8_attn`` takes: D % 8 == 0, D <= 256, GQA groups of 1 / 2 / 4 / 8."""
    return (head_dim % 8 == 0 and 0 < head_dim <= 256 and kv_heads > 0 and n_heads % kv_heads == 0
            and n_heads // kv_heads in GROUPS)


# --------------------------------------------------------------- contract
@torch.no_grad()
def quantize_rows(x: torch.Tensor):
    """x [..., D] -> (e4m3 bytes uint8 [..., D], scale fp32 [...]): ``quantize_weight`` on the rows."""
    w8 = quantize_weight(x.reshape(-1, x.shape[-1]))
    return w8.q.view(x.shape), w8.scale.view(x.shape[:-1])


def dequantize_rows(q: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``scale[...] * q[..., d]`` formed in fp32 (fp64 when asked for fp64), then cast."""
    ft = torch.float64 if dtype == torch.float64 else torch.float32
    return (q.view(torch.float8_e4m3fn).to(ft) * scale.to(ft)[..., None]).to(dtype)


def gather_kv8(cache: torch.Tensor, scale: torch.Tensor, seq: int, n: int, block_table=None, dtype=torch.float32):
    """``ops.decode.gather_kv`` of a byte cache, dequantized: tokens [0, n) of ``seq`` as [Hkv, n, D]."""
    q = gather_kv(cache, seq, n, block_table)
    s = gather_kv(scale[..., None], seq, n, block_table)[..., 0]
    return dequantize_rows(q, s, dtype)


@torch.no_grad()
def kv8_prep_reference(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, pos, slots, k_cache, v_cache,
                       k_scale, v_scale, block_table=None):
    """``ops.decode.decode_prep``'s semantics on a byte cache: RoPE in fp32, Q rotated in place exactly
    as there; the rotated K rounded to ``qkv.dtype`` (what the 16-bit cache would hold), then
    ``quantize_rows``; V quantized as it is."""
    H, Hkv, D = n_heads, kv_heads, head_dim
    x = _prep_rows_reference(qkv, H, Hkv, D, rot, interleaved, cos, sin, pos)
    sl, p = slots.long(), pos.long()
    if block_table is not None:
        PS = k_cache.shape[2]
        sl, p = block_table.long()[sl, p // PS], p % PS
    kq, ks = quantize_rows(x[:, H:H + Hkv].to(qkv.dtype))
    vq, vs = quantize_rows(x[:, H + Hkv:].to(qkv.dtype))
    k_cache[sl, :, p], k_scale[sl, :, p] = kq, ks
    v_cache[sl, :, p], v_scale[sl, :, p] = vq, vs


def kv8_attention_reference(q, k_cache, v_cache, k_scale, v_scale, slots, kv_lens, n_heads, scale, alibi=None,
                            out=None, block_table=None, window: int = 0, fp64: bool = False):
    """``ops.decode.decode_attention_reference`` over the dequantized cache (fp64 arithmetic when
    asked). Only rows of [max(0, L - window), L) are touched."""
    B = q.shape[0]
    _, Hkv, _, D = k_cache.shape
    H = n_heads
    ft = torch.float64 if fp64 else torch.float32
    if out is None:
        out = torch.empty(B, H * D, device=q.device, dtype=q.dtype)
    for b in range(B):
        n = int(kv_lens[b])
        lo = max(0, n - window) if window > 0 else 0
        s_ = int(slots[b])
        qb = q[b, :H * D].to(ft).view(H, D)
        kb = gather_kv8(k_cache, k_scale, s_, n, block_table, ft)[:, lo:].repeat_interleave(H // Hkv, 0)  # [H, n, D]
        vb = gather_kv8(v_cache, v_scale, s_, n, block_table, ft)[:, lo:].repeat_interleave(H // Hkv, 0)
        sc = torch.einsum("hd,hnd->hn", qb, kb) * scale
        if alibi is not None:
            sc = sc + alibi.to(ft)[:, None] * (torch.arange(lo, n, device=q.device) - (n - 1)).to(ft)[None]
        o = torch.einsum("hn,hnd->hd", sc.softmax(-1), vb)
        out[b] = o.reshape(-1).to(out.dtype)
    return out


# ------------------------------------------------------------- dispatching
def _native(x: torch.Tensor, k_cache: torch.Tensor, *symbols: str) -> bool:
    """GPU bf16 / fp16 tensors run the kernels; a missing kernel raises (no quiet reference path)."""
    if not (x.is_cuda and k_cache.is_cuda and x.dtype in (torch.bfloat16, torch.float16)):
        return False
    for sym in symbols:
        if not _lib.has(sym):
            _lib.require()
            raise RuntimeError(f"{sym} missing from the kernel library (rebuild: python tools/build_ext.py)")
    return True


def _check_cache(k_cache, v_cache, k_scale, v_scale):
    assert k_cache.dtype == torch.uint8 and v_cache.dtype == torch.uint8, "FP8 KV caches hold uint8 e4m3 bytes"
    assert k_scale.dtype == torch.float32 and v_scale.dtype == torch.float32
    assert k_cache.stride(-1) == 1 and k_cache.stride() == v_cache.stride() and k_cache.shape == v_cache.shape
    assert k_scale.shape == k_cache.shape[:-1] and v_scale.shape == k_scale.shape
    assert k_scale.stride(-1) == 1 and k_scale.stride() == v_scale.stride()


def kv8_prep(qkv: torch.Tensor, n_heads: int, kv_heads: int, head_dim: int, rot: int, interleaved: bool,
             cos: torch.Tensor | None, sin: torch.Tensor | None, pos: torch.Tensor, slots: torch.Tensor,
             k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
             block_table: torch.Tensor | None = None):
    """``ops.decode.decode_prep`` on a byte cache: rotates Q in place, writes the e4m3 rows and scales of
    each row b's K and V into cache[slots[b], :, pos[b]] (paged: into its page)."""
    _check_cache(k_cache, v_cache, k_scale, v_scale)
    if _native(qkv, k_cache, "kca_kv8_prep"):
        assert qkv.stride(-1) == 1 and pos.dtype == torch.int32 and slots.dtype == torch.int32
        tbl, tstride, shift = _table_args(block_table, k_cache)
        _lib.call("kca_kv8_prep", qkv.data_ptr(), qkv.stride(0), qkv.shape[0], n_heads, kv_heads, head_dim, rot,
                  int(interleaved), _lib.ptr(cos), _lib.ptr(sin), pos.data_ptr(), slots.data_ptr(),
                  k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(), k_cache.stride(0),
                  k_cache.stride(1), k_cache.stride(2), k_scale.stride(0), k_scale.stride(1), tbl, tstride, shift,
                  int(qkv.dtype == torch.float16), _lib.stream())
        return
    kv8_prep_reference(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, pos, slots, k_cache, v_cache,
                       k_scale, v_scale, block_table)


def kv8_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor,
                  v_scale: torch.Tensor, slots: torch.Tensor, kv_lens: torch.Tensor, n_heads: int, max_kv: int,
                  scale: float | None = None, alibi: torch.Tensor | None = None, out: torch.Tensor | None = None,
                  ws: torch.Tensor | None = None, chunk: int = 0, block_table: torch.Tensor | None = None,
                  window: int = 0) -> torch.Tensor:
    """``ops.decode.decode_attention`` over a byte cache. ``ws``: ``decode_ws_floats`` fp32 words (the
    16-bit kernel's sizing); allocated here when missing or short."""
    _check_cache(k_cache, v_cache, k_scale, v_scale)
    B = q.shape[0]
    _, Hkv, L, D = k_cache.shape
    H = n_heads
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty(B, H * D, device=q.device, dtype=q.dtype)
    if _native(q, k_cache, "kca_kv8_attn"):
        assert q.stride(-1) == 1 and out.stride(-1) == 1 and out.dtype == q.dtype
        assert q.stride(0) % 8 == 0 and q.data_ptr() % 16 == 0, "query rows must be 16-byte aligned"
        assert kv_lens.dtype == torch.int32 and slots.dtype == torch.int32
        tbl, tstride, shift = _table_args(block_table, k_cache)
        assert max_kv <= (L if block_table is None else block_table.shape[1] * L)
        if chunk <= 0:
            chunk = decode_chunk(B, Hkv, max_kv)
        need = decode_ws_floats(B, H, Hkv, D, max_kv, chunk)
        if need and (ws is None or ws.numel() < need):
            ws = torch.zeros(need, device=q.device, dtype=torch.float32)
        _lib.call("kca_kv8_attn", q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(),
                  k_scale.data_ptr(), v_scale.data_ptr(), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2),
                  k_scale.stride(0), k_scale.stride(1), slots.data_ptr(), kv_lens.data_ptr(), out.data_ptr(),
                  out.stride(0), _lib.ptr(ws), ws.numel() if ws is not None else 0, B, H, Hkv, D, max_kv, chunk,
                  float(scale), _lib.ptr(alibi), tbl, tstride, shift, int(window), int(q.dtype == torch.float16),
                  _lib.stream())
        return out
    return kv8_attention_reference(q, k_cache, v_cache, k_scale, v_scale, slots, kv_lens, H, scale, alibi, out,
                                   block_table, window)


def kv8_prep_attention(qkv: torch.Tensor, n_heads: int, kv_heads: int, head_dim: int, rot: int, interleaved: bool,
                       cos: torch.Tensor | None, sin: torch.Tensor | None, pos: torch.Tensor, slots: torch.Tensor,
                       k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                       kv_lens: torch.Tensor, max_kv: int, scale: float | None = None,
                       alibi: torch.Tensor | None = None, out: torch.Tensor | None = None,
                       ws: torch.Tensor | None = None, block_table: torch.Tensor | None = None,
                       window: int = 0) -> torch.Tensor:
    """``kv8_prep`` + ``kv8_attention`` for the decode step (kv_lens = pos + 1): on the GPU the prep
    launch, the attention launch and, past one split, the combine launch."""
    kv8_prep(qkv, n_heads, kv_heads, head_dim, rot, interleaved, cos, sin, pos, slots, k_cache, v_cache, k_scale,
             v_scale, block_table)
    return kv8_attention(qkv, k_cache, v_cache, k_scale, v_scale, slots, kv_lens, n_heads, max_kv, scale, alibi, out,
                         ws, block_table=block_table, window=window)


__all__ = ["quantize_rows", "dequantize_rows", "gather_kv8", "kv8_prep_reference", "kv8_attention_reference",
           "kv8_prep", "kv8_attention", "kv8_prep_attention", "supported", "GROUPS"]
