"""Model runner for serving: slot KV cache, prefill, fused decode step, HIP graphs.

The FT-equivalent decode loop for every causal LM in
``models.causal_lm`` (GPT-2, GPT-J, GPT-NeoX/Pythia, GPT-Neo, BLOOM):

* ``KVCache``: paged by default -- per layer a pool of [Hkv, 64, D] pages and a
  block table per sequence slot (head-major pages, so each (sequence, head,
  page) is a contiguous HBM stream); ``page_size=0`` gives one contiguous
  [Hkv, max_len, D] slot per sequence. 288 GB of HBM holds e.g. 64 GPT-J
  sequences x 2048 tokens (60 GB) next to the 12 GB of weights; with pages, the
  slot count is no longer tied to that worst case.
* ``prefill``: prompts (ragged: right-padded in one batch) through the
  flash-attention kernel, K/V (post-RoPE) written into each sequence's pages.
* ``decode``: one token per running sequence -- fused QKV GEMM ->
  ``kca_decode_prep`` (RoPE + cache append) -> ``kca_decode_attn`` (split-K) ->
  out-proj, residual adds fused into the next LayerNorm -> LM head ->
  ``kca_sample_logits``. On GPU the whole step (all layers + sampling) is
  captured once per (batch bucket, kv bucket) into a HIP graph and replayed, so
  a GPT-J step is one graph launch + one 8-byte/row D2H copy.

Host inputs of a step (tokens, positions, slots, sampling params, bans, seeds)
travel in ONE packed pinned buffer -> one H2D copy. ``decode_async`` launches a
step without waiting for it and can take each row's input token from the
previous launch's device output, so the engine launches step t+1 before it
reads step t's tokens (``LLMEngine``'s one-step lookahead).

``weight_dtype="fp8"`` (or ``KCA_DECODE_WEIGHTS=fp8`` when the keyword is None;
unset / ``0``: off, the default): FP8 weight-only decode. Every block's QKV,
out-projection, fc_in and fc_out weights are quantized once at construction
(``ops.w8.quantize_weight``: e4m3 bytes + one fp32 scale per output row) and every
decode step takes the per-projection path with those four projections on
``ln_rows`` + ``kca_w8_gemm``, streaming half the weight bytes. The LM head and
the embeddings stay 16-bit. Prefill keeps using the 16-bit weights, so both copies
stay resident: decode-time weight memory is 1.5x the 16-bit weights (2x with the
default packed twins of the matrix-core layer, which this mode does not build) --
unless ``prefill_weights="quantized"`` (below) releases them.

``weight_dtype="mxfp4"`` (``KCA_DECODE_WEIGHTS=mxfp4``): MXFP4 weight-only decode, the same
scheme one format further. The four projections of every block are quantized once
(``ops.mx4.quantize_weight``: e2m1 nibbles + one e8m0 scale byte per 32 consecutive
``k`` of an output row, 0.53 bytes per weight) and every decode step at every batch
size takes the per-projection path on ``ln_rows`` + ``kca_mx4_gemm``
(``csrc/kernels/gemv_mx4.hip``); ``mx4_steps`` counts those steps, and ``w8_steps``,
``fused_steps`` and ``batched_steps`` stay 0. The LM head, the embeddings and prefill
keep 16-bit weights. Composes with ``kv_dtype="fp8"``. Not covered: tensor-parallel
linears, layer-split placement, a projection with ``K % 32 != 0`` (``ValueError``).

``kv_dtype="fp8"`` (or ``KCA_DECODE_KV=fp8`` when the keyword is None; unset / ``0`` /
``none`` / ``off``: off, the default): FP8 KV cache. Every cached K / V row is stored as
e4m3 bytes plus one fp32 scale per (token, kv-head) (``ops.kv8``), (D + 4) / 2D of the
16-bit cache, and every decode step takes the per-projection path with the attention on
``kca_kv8_prep`` + ``kca_kv8_attn`` (``csrc/kernels/decode_kv8.hip``): the fused batch-1
layer and the matrix-core layer are not used in this mode. Prefill attends to the 16-bit
K / V of its own forward and quantizes only what it stores; chunked prefill sees the
earlier chunks dequantized (quantized values) and the current chunk exact. Composes with
``weight_dtype="fp8"``. Not covered: tensor-parallel and layer-split models, head dims
outside D % 8 == 0, D <= 256, GQA groups other than 1 / 2 / 4 / 8 (``ValueError``).

``spec_tokens=T`` (or ``KCA_DECODE_SPEC=T`` when the keyword is None; unset / ``0`` / ``none`` /
``off``: off, the default; T in 2 / 4 / 8): speculative decoding. ``verify`` / ``verify_async`` run one
step over up to T tokens per sequence -- its last token and up to T - 1 drafted ones -- as ``Bb * T``
rows of the ordinary layer code (the matrix-core layer while the rows fit it, the per-projection path
otherwise, so ``weight_dtype`` composes), with the attention on ``kca_spec_prep`` + ``kca_spec_attn``
(``csrc/kernels/decode_spec.hip``): the T queries of a sequence share every K/V row load. Every row is
sampled (its own seed and bans); the caller keeps the samples up to the first one that contradicts its
draft (``LLMEngine``). Rejected positions stay in the cache past the sequence's length and the next step
overwrites them. A bucket of T >= 4 whose KV stream is short (``KCA_DECODE_SPEC_ROWS_WORK``, default 65536
(sequence, kv-head, position) rows; 0: never) runs ``kca_spec_prep`` + ``kca_decode_attn`` on the rows
instead, where that measured faster (docs/PERF.md, Round 12). Each (batch, T, kv, sampler) bucket has its
own static buffers and its own graph, apart from the decode graphs; ``spec_steps`` counts the steps built
and ``step_launches[("spec", Bb, T)]`` their launches. Not covered (``ValueError``): T outside 2 / 4 / 8,
(H / Hkv) * T > 8, tensor-parallel and layer-split models, ``kv_dtype="fp8"``.

``prefill_weights="quantized"`` (or ``KCA_PREFILL_WEIGHTS=quantized`` when the keyword is None; unset / ``0`` /
``16bit`` / ``off``: off, the default; needs ``weight_dtype`` "fp8" or "mxfp4", ``ValueError`` otherwise, and
inherits that option's exclusions): prefill on the quantized weights too. ``prefill`` -- chunked prefill with
``start`` included -- runs the four projections of every block through ``ops.wq_gemm.wq_linear``
(``kca_wq_gemm``, csrc/kernels/gemm_wq.hip: one tiled matrix-core launch per projection, the MLP's
activation fused into fc_in's); LayerNorms, RoPE, cache writes, flash attention, the final LayerNorm and
the 16-bit LM head are as without the option, and so are decode and verify, which already run on the
quantized weights. A request then sees ONE model, and the 16-bit weights of the projections are released as
each is quantized: the parameter keeps its dtype and device with ``numel() == 0`` (the runner records its
shape), and calling the module directly raises a ``RuntimeError``. A projection ``weight`` may live on the
host when the runner is built (biases and everything else on the device): it is copied to the device one
projection at a time, quantized there and dropped, so peak device memory is the quantized model plus one
16-bit projection. ``weight_bytes()`` reports quantized / released / resident bytes and
``wq_prefill_steps`` counts the projection calls. Composes with ``kv_dtype="fp8"`` and ``spec_tokens``.

``prefix_cache=True`` (or ``KCA_PREFIX_CACHE=1`` when the keyword is None; unset / ``0`` / ``off``: off, the
default): prefix caching. The cache keeps an index of the full prompt pages it holds (``KVCache``) and
``adopt_prefix`` installs a matched chain of them, shared, as the first pages of a slot; ``prefill`` then
computes only the rest with ``start`` = the adopted length. With the option on, a continued prefill -- a
prefix hit or a chunk of ``prefill_chunk``, anything with a ``start`` > 0 in the batch -- runs ONE
``kca_prefill_paged_attn`` launch per layer for the whole ragged batch (``ops.prefill_paged``,
csrc/kernels/prefill_paged.hip: the flash-attention forward with its K/V tiles read through the block
table; bf16 and fp16) instead of gathering every row's keys into fresh tensors and attending row by row.
Layers the kernel does not cover (``ops.prefill_paged.supported``: GPT-Neo's local layers) keep that gather
loop, and so does the one shape at which it measured faster (``_paged_prefill``: a single bf16 row of
>= 512 queries behind >= 2048 cached tokens). ``paged_prefill_calls`` / ``gather_prefill_calls`` count the layer calls of either kind. With the
option off nothing changes. Composes with ``weight_dtype``, ``prefill_weights="quantized"``, ``spec_tokens``
and ``prefill_chunk``. Not covered (``ValueError``): ``page_size=0``, tensor-parallel and layer-split models,
and ``kv_dtype="fp8"`` -- a hit would see its prefix quantized where a miss sees it exact, so outputs would
depend on what the cache happens to hold; the kernel reads 16-bit pages only.
"""
from __future__ import annotations

import math
import os

import torch

from .. import ops
from ..ops import decode as dops
from ..ops import _lib
from ..ops import skinny_mm as smm
from ..ops.gemv import embed_ln_rows, ln_rows, ln_skinny_linear, skinny_linear
from ..ops import kv8
from ..ops import spec
from ..ops import prefill_paged
from ..ops.kv8 import quantize_rows
from ..ops import mx4
from ..ops.w8 import quantize_weight, w8_linear
from ..ops.wq_gemm import wq_linear

# decode steps: each row's RoPE angles and page-table row travel with the step's packed inputs (fixed
# device addresses), so every layer's attention chain loads them in its first memory round trip
# instead of after the length / slot arrive; KCA_DECODE_STEP_DESC=0: look them up on the device
_STEP_DESC = os.environ.get("KCA_DECODE_STEP_DESC", "1") not in ("0", "false")
# ... also for batch > 1 (the unfused per-layer path); KCA_DECODE_STEP_DESC_BATCHED=0: batch 1 only
_STEP_DESC_BATCHED = os.environ.get("KCA_DECODE_STEP_DESC_BATCHED", "1") not in ("0", "false")


def _next_pow2(n: int, lo: int = 1) -> int:
    p = lo
    while p < n:
        p *= 2
    return p


class KVCacheFull(RuntimeError):
    """No free KV page for a sequence (the engine's admission control keeps
    running requests clear of this)."""


class KVCache:
    """Per-layer K and V storage for the serving engine.

    ``page_size == 0``: contiguous slots [slots+1, Hkv, max_len, D] (a slot is
    one sequence's whole capacity). ``page_size > 0`` (default): paged pools
    [pages+1, Hkv, PS, D] plus a block table [slots+1, max_len/PS] (int32,
    device; host twin ``table_h``) -- a sequence holds only the pages it has
    filled, finished requests return theirs at once, and beams share their
    prefix pages (refcounted, ``fork`` copies only a partial tail page). The
    last page and the last table row are scratch: free table entries point at
    the scratch page, so a stray read or a graph bucket's padding row touches
    nothing live. Head-major pages keep each (sequence, head, page) a
    contiguous PS*D*2-byte stream for the decode kernel (``ops.decode``).

    ``kv_dtype="fp8"``: ``k`` / ``v`` hold OCP e4m3 bytes (uint8, the same shapes) and ``k_scale`` /
    ``v_scale`` (fp32, ``shape[:-1]``) one scale per (token, kv-head) row (``ops.kv8``): (D + 4) / 2D of
    the 16-bit cache's bytes. Pages, the block table, the scratch page / slot and ``fork`` work as above
    (scales travel with their rows). The default (None) is the 16-bit cache, with no scale tensors.

    Prefix index (``enable_prefix_index``; paged caches, ``ModelRunner(prefix_cache=True)``): full pages of
    prompts are registered under ``(parent page id or -1, the page's PS token ids)`` -- compared by value,
    so no hash collision can serve another prompt's K/V -- and ``lookup`` returns the longest registered
    chain of a prompt for ``adopt``. The index holds one reference per registered page; a page held by
    nobody else is evictable and counts as free (``free_count``): ``reserve`` and ``fork`` evict in LRU
    order (a use refreshes the whole chain; ties go deepest first, so a page never leaves before a page
    that extends it) when the free list runs short, and raise ``KVCacheFull`` only after that. A slot
    registers a page only under a parent it holds itself (registration stops at a key that another page
    already serves), so whoever holds a registered page holds its ancestors: the pages with no holder but
    the index are closed under "extends" and all of them can go.
    """

    def __init__(self, n_layers: int, slots: int, kv_heads: int, max_len: int, head_dim: int,
                 device, dtype=torch.bfloat16, page_size: int = 0, n_pages: int | None = None,
                 layer_devices: list | None = None, kv_dtype: str | None = None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"KVCache kv_dtype: {kv_dtype!r} (supported: 'fp8', or None)")
        self.kv_dtype = kv_dtype
        self.slots, self.max_len, self.scratch = slots, max_len, slots
        self.page_size = page_size
        self.device = torch.device(device)
        # layer-split models (parallel.layer_split): each layer's cache lives on that layer's device
        self.layer_devices = [torch.device(d) for d in layer_devices] if layer_devices else [self.device] * n_layers
        self.devices = list(dict.fromkeys([self.device] + self.layer_devices))
        if page_size:
            if page_size < 16 or page_size & (page_size - 1):
                raise ValueError(f"page_size {page_size}: need a power of two >= 16")
            self.blocks = -(-max_len // page_size)
            # default: every slot can hold a full-length sequence, plus one page per slot of headroom
            # for beam forks (a fork copies a partial tail page before the old one is dropped)
            self.n_pages = int(n_pages or slots * (self.blocks + 1))
            self.scratch_page = self.n_pages
            shape = (self.n_pages + 1, kv_heads, page_size, head_dim)
            self.table_h = torch.full((slots + 1, self.blocks), self.n_pages, dtype=torch.int32)
            self.tables = {d: self.table_h.to(d) for d in self.devices}
            self.table = self.tables[self.device]
            self.free_pages = list(range(self.n_pages - 1, -1, -1))
            self.ref = [0] * self.n_pages
            self.pages: list[list[int]] = [[] for _ in range(slots + 1)]
            self._dirty = False
        else:
            self.table = None
            self.n_pages = 0
            shape = (slots + 1, kv_heads, max_len, head_dim)
            self.tables = {}
        self._pidx = None  # prefix index: (parent page or -1, token tuple) -> page (enable_prefix_index)
        self.dtype = dtype  # the model's element type (an FP8 cache dequantizes to it for chunked prefill)
        if kv_dtype == "fp8":
            dtype = torch.uint8
        self.k = [torch.zeros(shape, device=d, dtype=dtype) for d in self.layer_devices]
        self.v = [torch.zeros(shape, device=d, dtype=dtype) for d in self.layer_devices]
        self.k_scale = self.v_scale = None
        if kv_dtype == "fp8":
            self.k_scale = [torch.zeros(shape[:-1], device=d, dtype=torch.float32) for d in self.layer_devices]
            self.v_scale = [torch.zeros(shape[:-1], device=d, dtype=torch.float32) for d in self.layer_devices]

    def _tensors(self):
        """Per layer, the tensors that hold its rows: (k, v) or (k, v, k_scale, v_scale)."""
        if self.k_scale is None:
            return list(zip(self.k, self.v))
        return list(zip(self.k, self.v, self.k_scale, self.v_scale))

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for ts in self._tensors() for t in ts)

    @property
    def paged(self) -> bool:
        return self.page_size > 0

    def pages_for(self, n_tokens: int) -> int:
        return -(-n_tokens // self.page_size) if self.paged else 0

    def free_count(self) -> int:
        if not self.paged:
            return 0
        return len(self.free_pages) + (len(self._evictable()) if self._pidx is not None else 0)

    # ---------------------------------------------------------- prefix index
    def enable_prefix_index(self):
        if not self.paged:
            raise ValueError("the prefix index needs a paged cache (page_size > 0)")
        self._pidx = {}
        self._pinfo: dict = {}  # page -> [key, depth, last use]
        self._ptick = 0
        self.prefix_registered = 0  # pages ever registered
        self.prefix_evictions = 0

    def _evictable(self) -> list[int]:
        """Registered pages nobody but the index holds (class docstring: all of them can go)."""
        return [pg for pg in self._pinfo if self.ref[pg] == 1]

    def _evict(self, n: int):
        """Up to ``n`` index-only pages back to the free list, least recently used and deepest first."""
        victims = sorted(self._evictable(), key=lambda pg: (self._pinfo[pg][2], -self._pinfo[pg][1]))[:n]
        for pg in victims:
            del self._pidx[self._pinfo.pop(pg)[0]]
            self.prefix_evictions += 1
        self._drop(victims)

    def lookup(self, tokens: list, max_pages: int) -> list[int]:
        """The longest registered chain of full pages of ``tokens`` (at most ``max_pages``), refreshed."""
        PS, parent, chain = self.page_size, -1, []
        for i in range(min(max_pages, len(tokens) // PS)):
            pg = self._pidx.get((parent, tuple(tokens[i * PS:(i + 1) * PS])))
            if pg is None:
                break
            chain.append(pg)
            parent = pg
        self._touch(chain)
        return chain

    def clear_prefix_index(self):
        """Every page nobody but the index holds goes back to the free list."""
        self._evict(len(self._pinfo))

    def _touch(self, chain):
        self._ptick += 1
        for pg in chain:
            self._pinfo[pg][2] = self._ptick

    def register(self, slot: int, tokens: list, n_pages: int) -> int:
        """Pages [0, n_pages) of ``slot`` -- full, holding ``tokens[:n_pages * PS]`` -- into the index.
        A key that is present keeps its page; registration stops where that page is not the slot's own.
        Returns the number of pages added."""
        PS, parent, chain, added = self.page_size, -1, [], 0
        own = self.pages[slot]
        for i in range(min(n_pages, len(own), len(tokens) // PS)):
            key = (parent, tuple(tokens[i * PS:(i + 1) * PS]))
            pg = self._pidx.get(key)
            if pg is None:
                pg = own[i]
                if pg in self._pinfo:  # already serves another key (its old parent was evicted)
                    break
                self._pidx[key] = pg
                self._pinfo[pg] = [key, i, 0]
                self.ref[pg] += 1
                added += 1
            elif pg != own[i]:
                break
            chain.append(pg)
            parent = pg
        self._touch(chain)
        self.prefix_registered += added
        return added

    def adopt(self, slot: int, pages: list[int]):
        """``pages`` (a ``lookup`` chain) become the first pages of the empty ``slot``, shared."""
        assert self.paged and not self.pages[slot]
        for pg in pages:
            self.ref[pg] += 1
        self.pages[slot] = list(pages)
        if pages:
            self.table_h[slot, :len(pages)] = torch.tensor(pages, dtype=torch.int32)
            self._dirty = True

    # ------------------------------------------------------------ page table
    def reserve(self, slot: int, n_tokens: int):
        """Make positions [0, n_tokens) of ``slot`` addressable (allocates pages)."""
        if not self.paged:
            return
        own = self.pages[slot]
        need = self.pages_for(min(n_tokens, self.max_len)) - len(own)
        if need <= 0:
            return
        if len(self.free_pages) < need <= self.free_count():  # (a request that cannot fit evicts nothing)
            self._evict(need - len(self.free_pages))
        if need > len(self.free_pages):
            raise KVCacheFull(f"slot {slot} needs {need} KV pages, {len(self.free_pages)} free")
        for _ in range(need):
            pg = self.free_pages.pop()
            self.ref[pg] = 1
            self.table_h[slot, len(own)] = pg
            own.append(pg)
        self._dirty = True

    def _drop(self, pages):
        for pg in pages:
            self.ref[pg] -= 1
            if self.ref[pg] == 0:
                self.free_pages.append(pg)

    def release(self, slot: int):
        if not self.paged or not self.pages[slot]:
            return
        self._drop(self.pages[slot])
        self.pages[slot] = []
        self.table_h[slot].fill_(self.scratch_page)
        self._dirty = True

    def sync(self):
        """Block-table edits -> device (stream-ordered after the work already queued)."""
        if self.paged and self._dirty:
            for t in self.tables.values():
                t.copy_(self.table_h)
            self._dirty = False

    def table_on(self, dev):
        return self.tables.get(torch.device(dev)) if self.paged else None

    def _per_layer(self, idx: list[int]):
        """``idx`` as a long tensor on every cache device."""
        t = torch.tensor(idx, dtype=torch.long)
        return {d: t.to(d) for d in self.devices}

    def fork(self, dst: list[int], src: list[int], upto: int):
        """Sequence ``src[i]`` positions [0, upto) -> ``dst[i]``. Paged: whole
        pages are shared (refcount), only a partial last page is copied; a
        permutation (dst and src overlapping) is safe."""
        if not dst:
            return
        if not self.paged:
            d, s = self._per_layer(dst), self._per_layer(src)
            for ts, dev in zip(self._tensors(), self.layer_devices):
                for t in ts:  # (FP8: the scales of the prefix with its rows)
                    t[d[dev], :, :upto] = t[s[dev], :, :upto]  # RHS gathered first: overlapping permutations are safe
            return
        full, part = divmod(upto, self.page_size)
        new_lists, cp_from, cp_to = [], [], []
        for d_, s_ in zip(dst, src):
            shared = self.pages[s_][:full]
            for pg in shared:
                self.ref[pg] += 1
            lst = list(shared)
            if part:
                if not self.free_pages and self._pidx is not None:
                    self._evict(1)
                if not self.free_pages:
                    self._drop([pg for l_ in new_lists for pg in l_] + lst)
                    raise KVCacheFull("no free KV page for a beam fork")
                pg = self.free_pages.pop()
                self.ref[pg] = 1
                cp_from.append(self.pages[s_][full])
                cp_to.append(pg)
                lst.append(pg)
            new_lists.append(lst)
        if cp_to:
            a, b = self._per_layer(cp_from), self._per_layer(cp_to)
            for ts, dev in zip(self._tensors(), self.layer_devices):
                for t in ts:  # (FP8: the tail page's scales with its rows)
                    t[b[dev]] = t[a[dev]]
        for d_, lst in zip(dst, new_lists):  # old dst pages go only after every source was read
            self._drop(self.pages[d_])
            self.pages[d_] = lst
            self.table_h[d_].fill_(self.scratch_page)
            if lst:
                self.table_h[d_, :len(lst)] = torch.tensor(lst, dtype=torch.int32)
        self._dirty = True

    # --------------------------------------------------------------- prefill
    def plan_write(self, slots: list[int], lens: list[int], T: int, start: list[int] | None = None):
        """Index plan for writing prompts (right-padded to T) into the cache;
        ``start``: first position of each row (chunked prefill continues a slot)."""
        if not self.paged:
            return None
        import numpy as np
        PS = self.page_size
        start = start or [0] * len(slots)
        pg, off, src = [], [], []
        for i, (s_, L, p0) in enumerate(zip(slots, lens, start)):
            t = np.arange(p0, p0 + L)
            own = np.asarray(self.pages[s_][:self.pages_for(p0 + L)], dtype=np.int64)
            pg.append(own[t // PS])
            off.append(t % PS)
            src.append(i * T + t - p0)
        host = [torch.from_numpy(np.concatenate(xs)) for xs in (pg, off, src)]
        return {d: tuple(t.to(d) for t in host) for d in self.devices}

    def write(self, li: int, k: torch.Tensor, v: torch.Tensor, slots: list[int], lens: list[int], plan,
              start: list[int] | None = None):
        """k, v: [n, T, Hkv, D] (strided views of the QKV GEMM output). FP8 cache: the rows are
        quantized here in torch (``ops.kv8.quantize_rows``; prefill is not the hot path) and bytes and
        scales take the same plan."""
        kc, vc = self.k[li], self.v[li]
        if self.k_scale is not None:
            (k, ks), (v, vs) = quantize_rows(k), quantize_rows(v)
            ksc, vsc = self.k_scale[li], self.v_scale[li]
            if plan is None:
                start = start or [0] * len(slots)
                for i, (s_, L, p0) in enumerate(zip(slots, lens, start)):
                    ksc[s_, :, p0:p0 + L].copy_(ks[i, :L].transpose(0, 1))
                    vsc[s_, :, p0:p0 + L].copy_(vs[i, :L].transpose(0, 1))
            else:
                pg, off, src = plan[self.layer_devices[li]]
                ksc[pg, :, off] = ks.reshape(-1, ks.shape[-1])[src]
                vsc[pg, :, off] = vs.reshape(-1, vs.shape[-1])[src]
        if plan is None:
            start = start or [0] * len(slots)
            for i, (s_, L, p0) in enumerate(zip(slots, lens, start)):  # strided copies (index scatter is ~4x slower)
                kc[s_, :, p0:p0 + L].copy_(k[i, :L].transpose(0, 1))
                vc[s_, :, p0:p0 + L].copy_(v[i, :L].transpose(0, 1))
            return
        pg, off, src = plan[self.layer_devices[li]]
        n, T, Hkv, D = k.shape
        kc[pg, :, off] = k.reshape(n * T, Hkv, D)[src]
        vc[pg, :, off] = v.reshape(n * T, Hkv, D)[src]


class _Packed:
    """Several small typed arrays in one byte buffer: two pinned host buffers
    (alternating per launch, so the host fills one while the previous launch's
    H2D copy may still be pending) + one device twin the decode graph reads."""

    def __init__(self, fields, device):
        self.off, self.fields = {}, fields
        o = 0
        for name, (dt, n) in fields.items():
            o = (o + 7) // 8 * 8
            self.off[name] = o
            o += n * torch.empty(0, dtype=dt).element_size()
        self.nbytes = (o + 7) // 8 * 8
        pin = device.type == "cuda"
        self.hosts = [torch.zeros(self.nbytes, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
        self.dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        # numpy views of the pinned host buffers: per-row scalar writes cost
        # ~0.1 us instead of a torch indexing op (~5 us) each
        self._nps = [{name: self._view(h, name).numpy() for name in fields} for h in self.hosts]
        self.cur = 0

    def flip(self):
        self.cur ^= 1

    @property
    def host(self):
        return self.hosts[self.cur]

    @property
    def np(self):
        return self._nps[self.cur]

    def _view(self, buf, name):
        dt, n = self.fields[name]
        o = self.off[name]
        es = torch.empty(0, dtype=dt).element_size()
        return buf[o:o + n * es].view(dt)

    def h(self, name):
        return self._view(self.host, name)

    def d(self, name):
        return self._view(self.dev, name)

    def upload(self):
        self.dev.copy_(self.host, non_blocking=True)


class DecodeHandle:
    """A launched decode step: its sampled ids / log-probs land in pinned host
    memory behind an event; ``result()`` waits for them. ``ids_dev`` is the
    device output the next launch may chain its input tokens from."""

    __slots__ = ("ids_h", "lps_h", "n", "event", "ids_dev", "_res")

    def __init__(self, ids_h, lps_h, n, event, ids_dev):
        self.ids_h, self.lps_h, self.n, self.event, self.ids_dev = ids_h, lps_h, n, event, ids_dev
        self._res = None

    def result(self):
        if self._res is None:
            if self.event is not None:
                self.event.synchronize()
            self._res = (self.ids_h[:self.n].tolist(), self.lps_h[:self.n].tolist())
        return self._res


class VerifyHandle:
    """A launched verify step; ``result()`` waits for it: (ids, logprobs), per row the samples of its
    n tokens (``ModelRunner.verify``)."""

    __slots__ = ("handle", "ns", "T")

    def __init__(self, handle, ns, T):
        self.handle, self.ns, self.T = handle, ns, T

    def result(self):
        ids, lps = self.handle.result()
        T = self.T
        return ([ids[i * T:i * T + k] for i, k in enumerate(self.ns)],
                [lps[i * T:i * T + k] for i, k in enumerate(self.ns)])


class ModelRunner:
    def __init__(self, model, max_slots: int = 32, max_len: int | None = None, use_graphs: bool | None = None,
                 max_bans: int = 16, page_size: int | None = None, kv_pages: int | None = None,
                 weight_dtype: str | None = None, kv_dtype: str | None = None, spec_tokens: int | str | None = None,
                 prefill_weights: str | None = None, prefix_cache: bool | str | None = None):
        self.model = model.eval()
        cfg = model.cfg
        self.cfg = cfg
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.max_len = max_len or cfg.max_pos
        # local heads: a tensor-parallel shard holds H/tp of them (parallel.tensor_parallel)
        self.H = model.h[0].attn.n_heads
        self.Hkv = self.H * cfg.kv_heads // cfg.n_heads
        self.D = cfg.head_dim
        self.V = cfg.vocab_size
        if page_size is None:
            page_size = int(os.environ.get("KCA_KV_PAGE_SIZE", "64"))
        # layer-split placement (parallel.layer_split): per-layer devices, the head's device
        self.layer_devs = [blk.ln_1.weight.device for blk in model.h]
        self.head_dev = model.ln_f.weight.device
        self.multi_device = len({str(d) for d in self.layer_devs + [self.device, self.head_dev]}) > 1
        self._wq_prefill = self._prefill_weights(prefill_weights)  # prefill on the quantized weights (module docstring)
        self.released: dict = {}  # id(linear) -> the shape of its released 16-bit weight
        self.wq_prefill_steps = 0  # prefill projections run on the quantized weights
        self._w8, self._mx4 = self._quantize_decode_weights(weight_dtype)
        self.w8_steps = 0  # decode steps built on the FP8 weights (eager runs and graph captures)
        self.mx4_steps = 0  # ... on the MXFP4 weights
        self._kv8 = self._kv_dtype(kv_dtype) == "fp8"
        self.kv8_steps = 0  # decode steps built on the FP8 KV cache (eager runs and graph captures)
        self.spec_tokens = self._spec_tokens(spec_tokens)  # T rows per sequence of a verify step (0: off)
        self.spec_steps = 0  # verify steps built (eager runs and graph captures)
        self._spec = None  # the per-sequence arrays of the verify step being built (_attn)
        # a verify bucket of T >= 4 with at most this many (sequence, kv-head, position) cache rows runs its
        # attention as Bb * T rows of the one-token kernel (_spec_rows); 0: the multi-token kernel always
        self._spec_rows_work = int(os.environ.get("KCA_DECODE_SPEC_ROWS_WORK", "65536"))
        self.spec_rows_steps = 0  # verify steps built on that arm
        self.prefix_cache = self._prefix_cache(prefix_cache, page_size)  # prefix caching (module docstring)
        self.paged_prefill_calls = 0  # continued-prefill layer calls on kca_prefill_paged_attn
        self.gather_prefill_calls = 0  # ... on the gather loop (_continued_attention)
        self.cache = KVCache(cfg.n_layers, max_slots, self.Hkv, self.max_len, self.D, self.device, self.dtype,
                             page_size=page_size, n_pages=kv_pages, layer_devices=self.layer_devs,
                             kv_dtype="fp8" if self._kv8 else None)
        if self.prefix_cache:
            self.cache.enable_prefix_index()
        self.max_slots = max_slots
        self.rot = cfg.rotary_dim
        self._rope = {}
        for d in self.cache.devices:
            self._rope[d] = ops.rope_tables(self.rot, self.max_len, cfg.rotary_base, d) if self.rot > 0 else (None, None)
        self.cos, self.sin = self._rope[self.device]
        self._rope_h = (self.cos.cpu().numpy(), self.sin.cpu().numpy()) if self.rot > 0 else None
        self._step_desc = None
        self.seen = torch.zeros(max_slots + 1, self.V, dtype=torch.uint8, device=self.device)
        self.max_bans = max_bans
        on_gpu = self.device.type == "cuda"
        if on_gpu:  # MI355X-tuned hipBLASLt/rocBLAS choices for the batched decode GEMMs (utils/tunable.py)
            from ..utils import tunable
            tunable.ensure(tunable.DECODE_FILE)
        self.use_graphs = on_gpu if use_graphs is None else (use_graphs and on_gpu)
        if self.multi_device:
            self.use_graphs = False  # one graph cannot span devices; the split path runs eagerly
        self._graphs: dict = {}
        self._pool = None
        self._static: dict = {}
        # parallel-residual models (GPT-J, NeoX): the MLP branch does not depend on attention, so at
        # decode its two weight-streaming GEMVs run on a side stream while the latency-bound attention
        # chain (split-K attention, combine, out-proj) runs on the main one -- both captured into the
        # step's graph as a fork/join. Not under TP: two concurrent collectives could interleave
        # differently across ranks.
        from ..parallel.tensor_parallel import RowParallelLinear
        from ..parallel.tp_emulation import is_emulated
        rows = [mm for mm in model.modules() if isinstance(mm, RowParallelLinear)]
        tp = bool(rows)
        # one rank of a TP layout on one GPU (parallel/tp_emulation.py): its collectives are local
        # stand-ins, so the fused single-device layer applies to its shard shapes
        tp_local = all(is_emulated(mm.group) for mm in rows)
        self._par_mlp = (cfg.parallel_residual and on_gpu and not tp and not self.multi_device
                         and os.environ.get("KCA_DECODE_PAR_MLP", "1") not in ("0", "false"))
        self._side = torch.cuda.Stream(device=self.device) if self._par_mlp else None
        # batch-1 decode layer on ONE queue, the residual add and the next LayerNorm in the tail of the
        # projection that produces it (ops/decode.py gemv_dual_ln), no LayerNorm launch of its own:
        #   "gptj" parallel residual, one shared LN: QKV GEMV -> attention + fc_in -> out + fc_out + LN
        #   "neox" parallel residual, ln_1 / ln_2 of the same h: as gptj, the tail writes both norms
        #   "seq"  sequential residual (BLOOM, GPT-2, GPT-Neo): QKV GEMV -> attention -> out-proj +
        #          residual + ln_2 -> fc_in GEMV -> fc_out + residual + next ln_1
        # KCA_DECODE_FUSED=0: the per-projection path (two-stream for parallel-residual models)
        ln2 = [blk.ln_2 for blk in model.h]
        self._layer_kind = ("gptj" if all(x is None for x in ln2) else "neox") if cfg.parallel_residual else "seq"
        # a real TP group (BLOOM TP=8 serving): sequential layers close each row-parallel projection with
        # the custom all-reduce's fused residual + LayerNorm tail (parallel/custom_ar.py res_ln)
        # (an emulated rank -- parallel/tp_emulation.py -- whose group has a rank-local custom all-reduce
        # registered runs the same kernels: bench/bloom_tp_bench.py measures the deployment's launches)
        self._tp_ar = None
        if (tp and self._layer_kind == "seq"
                and os.environ.get("KCA_TP_FUSED_TAIL", "1") not in ("0", "false")):
            from ..parallel.custom_ar import lookup
            ars = {id(mm.group): lookup(mm.group) for mm in rows}
            if len(ars) == 1 and None not in ars.values():
                self._tp_ar = next(iter(ars.values()))
        self._fused_ok = (on_gpu and not self.multi_device and (not tp or tp_local or self._tp_ar is not None)
                          and os.environ.get("KCA_DECODE_FUSED", "1") not in ("0", "false")
                          and cfg.hidden <= 16384
                          and (self._layer_kind != "neox"
                               or all(x.eps == blk.ln_1.eps for x, blk in zip(ln2, model.h)))
                          and (self._layer_kind == "seq"
                               or (self.H == self.Hkv and self.D % 8 == 0 and 64 < self.D <= 256)))
        self._fz: dict = {}
        self.step_launches: dict = {}
        self._outbufs: dict = {}
        self._chain_src = None
        # the fused step head gathers the token embedding itself (no learned positions / scale / LN on
        # the embedding) and resolves chained tokens on the device: KCA_DECODE_EMBED_HEAD=0 keeps the
        # torch embedding + cast + LN launches
        # (BLOOM's embedding LayerNorm: the gather kernel normalises with it, one ln_rows launch follows)
        self._embed_head = (self._fused_ok and getattr(model, "wpe", None) is None and cfg.embed_scale == 1.0
                            and os.environ.get("KCA_DECODE_EMBED_HEAD", "1") not in ("0", "false"))
        # batch 2..64: the matrix-core decode layer (ops/skinny_mm.py): every projection one weight-streaming
        # MFMA launch with its epilogue fused -- LayerNorm applied to the activation on load from the row
        # statistics the previous residual projection published, bias + GELU, bias + residual -- so the
        # layer loop has no LayerNorm, bias or hipBLASLt launch (parallel residual: [QKV | fc_in] one launch,
        # out-proj + fc_out one K-concatenated launch). KCA_DECODE_FUSED_BATCHED=0: per-projection path.
        d_model = cfg.hidden
        self.batched_steps = 0
        self._packs = {}  # packed weight twins of the matrix-core layer (_packed_w)
        self.fused_steps = 0  # batch-1 fused-layer steps built (eager runs and graph captures)
        # (real TP: sequential layers only -- each row-parallel projection closed by the custom all-reduce's
        # residual + row-statistics tail, parallel/custom_ar.py res_stats)
        # fp16 (the precision FasterTransformer / DS-Inference serve, BASELINE config 4) runs the same two
        # layers: every decode kernel (GEMVs, fused tails, attention, LayerNorm rows, MFMA layer, all-reduce
        # tails, sampler) has an fp16 instantiation (the *_f16 entry points)
        self._batched_ok = (self._fused_ok and self.dtype in (torch.bfloat16, torch.float16)
                            and d_model % 64 == 0 and d_model <= 16384
                            and os.environ.get("KCA_DECODE_FUSED_BATCHED", "1") not in ("0", "false"))
        # largest batch bucket the matrix-core layer takes, per layer kind, from same-box A/Bs against the
        # per-projection path (hipBLASLt + the fused LN / GELU / all-reduce launches,
        # profiles/decode_suite_r6_batched_vs_unfused.jsonl): GPT-J 3.49 vs 3.88 ms at B=16 but 4.63 vs
        # 4.27 at 32 (the per-projection step overlaps the MLP GEMMs with the attention on a side stream);
        # BLOOM TP=8 rank 11.46 vs 12.58 at 16, 14.25 vs 13.50 at 32 (hipBLASLt streams the 14336-wide
        # shapes faster from M = 32); NeoX wins at every batch (12.84 vs 15.86 at 32, 25.9 vs 28.3 at 64)
        # fp16 takes the same caps since the per-projection path's LayerNorm / GELU run their fp16
        # instantiations (ln_rows, kca_gelu_fwd_f16) instead of eager kernels: B=32 GPT-J 4.40 vs 4.65 ms,
        # BLOOM rank 13.38 vs 14.84 per-projection vs matrix-core layer (profiles/decode_fp16_cap_ab_r6.jsonl)
        self._batched_max_b = int(os.environ.get("KCA_DECODE_BATCHED_MAX_B", "0")) or \
            {"gptj": 16, "seq": 16}.get(self._layer_kind, 64)

    def _kv_dtype(self, kv_dtype):
        """FP8 KV cache (module docstring): "fp8" or None, from the keyword or KCA_DECODE_KV."""
        if kv_dtype is None:
            kv_dtype = os.environ.get("KCA_DECODE_KV", "") or None
        if kv_dtype in (None, "0", "none", "off"):
            return None
        if kv_dtype != "fp8":
            raise ValueError(f"kv_dtype / KCA_DECODE_KV: {kv_dtype!r} (supported: 'fp8', or unset)")
        from ..parallel import tensor_parallel as tpm
        tp_types = tuple(t for t in (getattr(tpm, n, None) for n in
                                     ("RowParallelLinear", "ColumnParallelLinear", "ParallelLMHead")) if t)
        if any(isinstance(mm, tp_types) for mm in self.model.modules()):
            raise ValueError("kv_dtype='fp8' (KCA_DECODE_KV=fp8) does not cover tensor-parallel models; "
                             "serve this model with the 16-bit KV cache")
        if self.multi_device:
            raise ValueError("kv_dtype='fp8' (KCA_DECODE_KV=fp8) does not cover a layer-split placement; "
                             "serve this model with the 16-bit KV cache")
        if not kv8.supported(self.D, self.H, self.Hkv):
            raise ValueError(f"kv_dtype='fp8' (KCA_DECODE_KV=fp8) does not cover head_dim {self.D} with "
                             f"{self.H} query / {self.Hkv} KV heads (needs head_dim % 8 == 0, <= 256, and "
                             f"{kv8.GROUPS} query heads per KV head); serve this model with the 16-bit KV cache")
        return "fp8"

    def _spec_tokens(self, spec_tokens) -> int:
        """Speculative decoding (module docstring): T in {2, 4, 8} or 0, from the keyword or KCA_DECODE_SPEC."""
        if spec_tokens is None:
            spec_tokens = os.environ.get("KCA_DECODE_SPEC", "") or None
        if spec_tokens is None or spec_tokens is False or str(spec_tokens).strip().lower() in ("0", "none", "off"):
            return 0
        opt = f"spec_tokens / KCA_DECODE_SPEC: {spec_tokens!r}"
        try:
            T = int(spec_tokens)
        except (TypeError, ValueError):
            raise ValueError(f"{opt} (supported: 2, 4, 8, or unset)") from None
        if T not in (2, 4, 8) or isinstance(spec_tokens, float):
            raise ValueError(f"{opt} (supported: 2, 4, 8, or unset)")
        from ..parallel import tensor_parallel as tpm
        tp_types = tuple(t for t in (getattr(tpm, n, None) for n in
                                     ("RowParallelLinear", "ColumnParallelLinear", "ParallelLMHead")) if t)
        if any(isinstance(mm, tp_types) for mm in self.model.modules()):
            raise ValueError(f"{opt} does not cover tensor-parallel models; serve this model without speculation")
        if self.multi_device:
            raise ValueError(f"{opt} does not cover a layer-split placement; serve this model without speculation")
        if self._kv8:
            raise ValueError(f"{opt} does not cover kv_dtype='fp8' (KCA_DECODE_KV=fp8): the multi-token attention "
                             "kernel reads the 16-bit KV cache")
        G = self.H // max(self.Hkv, 1)
        if G * T > 8:
            raise ValueError(f"{opt} with {G} query heads per KV head: the verify attention holds at most 8 "
                             f"queries per KV head (T <= {max(8 // G, 1)})")
        if not spec.supported(self.D, self.H, self.Hkv, T):
            raise ValueError(f"{opt} does not cover head_dim {self.D} with {self.H} query / {self.Hkv} KV heads "
                             "(needs head_dim % 8 == 0, <= 256, and (H / Hkv) * T in 2 / 4 / 8)")
        return T

    def _prefix_cache(self, prefix_cache, page_size: int) -> bool:
        """Prefix caching (module docstring): from the keyword or KCA_PREFIX_CACHE."""
        if prefix_cache is None:
            prefix_cache = os.environ.get("KCA_PREFIX_CACHE", "") or None
        if prefix_cache is None or prefix_cache is False or str(prefix_cache).strip().lower() in ("0", "none", "off"):
            return False
        if prefix_cache is not True and str(prefix_cache).strip().lower() not in ("1", "on", "true"):
            raise ValueError(f"prefix_cache / KCA_PREFIX_CACHE: {prefix_cache!r} (supported: True / 1, or unset)")
        opt = "prefix_cache=True (KCA_PREFIX_CACHE=1)"
        if not page_size:
            raise ValueError(f"{opt} needs the paged KV cache (page_size > 0): shared prefixes are shared pages")
        from ..parallel import tensor_parallel as tpm
        tp_types = tuple(t for t in (getattr(tpm, n, None) for n in
                                     ("RowParallelLinear", "ColumnParallelLinear", "ParallelLMHead")) if t)
        if any(isinstance(mm, tp_types) for mm in self.model.modules()):
            raise ValueError(f"{opt} does not cover tensor-parallel models; serve this model without it")
        if self.multi_device:
            raise ValueError(f"{opt} does not cover a layer-split placement; serve this model without it")
        if self._kv8:
            raise ValueError(f"{opt} does not cover kv_dtype='fp8' (KCA_DECODE_KV=fp8): a hit would see its prefix "
                             "quantized where a miss sees it exact, and the paged prefill kernel reads the 16-bit "
                             "KV cache")
        return True

    def _quantize_decode_weights(self, weight_dtype):
        """Weight-only decode (module docstring): ``({id(linear): W8Weight} | None, {id(linear):
        MX4Weight} | None)`` of every block's four projections -- FP8, MXFP4, or both None with the
        option off."""
        if weight_dtype is None:
            weight_dtype = os.environ.get("KCA_DECODE_WEIGHTS", "") or None
        if weight_dtype in (None, "0", "none", "off"):
            if self._wq_prefill:
                raise ValueError("prefill_weights='quantized' (KCA_PREFILL_WEIGHTS=quantized) needs weight_dtype "
                                 "'fp8' or 'mxfp4' (KCA_DECODE_WEIGHTS): there are no quantized weights to prefill on")
            return None, None
        if weight_dtype not in ("fp8", "mxfp4"):
            raise ValueError(f"weight_dtype / KCA_DECODE_WEIGHTS: {weight_dtype!r} "
                             "(supported: 'fp8', 'mxfp4', or unset)")
        opt = f"weight_dtype='{weight_dtype}' (KCA_DECODE_WEIGHTS={weight_dtype})"
        from ..parallel import tensor_parallel as tpm
        tp_types = tuple(t for t in (getattr(tpm, n, None) for n in
                                     ("RowParallelLinear", "ColumnParallelLinear", "ParallelLMHead")) if t)
        if any(isinstance(mm, tp_types) for mm in self.model.modules()):
            raise ValueError(f"{opt} does not cover tensor-parallel linears; "
                             "serve this model with 16-bit weights")
        if self.multi_device:
            raise ValueError(f"{opt} does not cover a layer-split placement; "
                             "serve this model with 16-bit weights")
        mods = [mod for blk in self.model.h for mod in (blk.attn.qkv, blk.attn.out, blk.mlp.fc_in, blk.mlp.fc_out)]
        if weight_dtype == "mxfp4":
            for mod in mods:
                if mod.weight.shape[1] % mx4.BLOCK:
                    raise ValueError(f"{opt} does not cover a projection with K = {mod.weight.shape[1]} "
                                     f"(MXFP4 blocks are {mx4.BLOCK} wide: K % {mx4.BLOCK} == 0); "
                                     "serve this model with 16-bit weights")
        quant = quantize_weight if weight_dtype == "fp8" else mx4.quantize_weight
        if not self._wq_prefill:
            qs = {id(mod): quant(mod.weight) for mod in mods}
        else:  # one projection at a time: to the device if it lives on the host, quantized, released
            qs = {}
            for mod in mods:
                qs[id(mod)] = quant(mod.weight.detach().to(self.device))
                self._release(mod)
        return (qs, None) if weight_dtype == "fp8" else (None, qs)

    def _prefill_weights(self, prefill_weights) -> bool:
        """``prefill_weights`` (module docstring): True for "quantized", from the keyword or
        KCA_PREFILL_WEIGHTS."""
        if prefill_weights is None:
            prefill_weights = os.environ.get("KCA_PREFILL_WEIGHTS", "") or None
        if prefill_weights in (None, "0", "16bit", "off"):
            return False
        if prefill_weights != "quantized":
            raise ValueError(f"prefill_weights / KCA_PREFILL_WEIGHTS: {prefill_weights!r} "
                             "(supported: 'quantized', '16bit', or unset)")
        return True

    def _release(self, mod):
        """Drop a quantized projection's 16-bit weight: the parameter stays, with its dtype and device and
        no elements; its shape goes to ``released``; calling the module raises."""
        w = mod.weight
        self.released[id(mod)] = (tuple(w.shape), w.element_size())
        w.data = torch.empty(0, dtype=w.dtype, device=w.device)
        if getattr(mod, "weight_t", None) is not None:
            mod.weight_t = None

        def refuse(module, args):
            raise RuntimeError(f"{type(module).__name__}{self.released[id(module)][0]}: its 16-bit weight was released "
                               "by prefill_weights=\"quantized\" (the runner prefills and decodes on the quantized "
                               "weights); call the runner, not the module")

        mod.register_forward_pre_hook(refuse)

    def weight_bytes(self) -> dict:
        """Bytes of the quantized projections, of the 16-bit weights released for them, and of every
        parameter the model still holds."""
        qs = self._w8 if self._w8 is not None else (self._mx4 or {})
        return {"quantized": sum(q.nbytes() for q in qs.values()),
                "released_16bit": sum(math.prod(shape) * es for shape, es in self.released.values()),
                "resident_16bit": sum(p_.numel() * p_.element_size() for p_ in self.model.parameters())}

    def _plin(self, mod, x, act: int = 0):
        """A prefill projection: the module, or -- ``prefill_weights="quantized"`` -- ``wq_linear`` on its
        quantized weight with the activation fused."""
        if not self._wq_prefill:
            return mod(x)
        w = (self._w8 if self._w8 is not None else self._mx4)[id(mod)]
        self.wq_prefill_steps += 1
        return wq_linear(x.reshape(-1, x.shape[-1]), w, mod.bias, act).view(*x.shape[:-1], -1)

    def _pmlp(self, mlp, x):
        if not self._wq_prefill:
            return mlp(x)
        act = 1 if mlp.approx in ("tanh", True) else 2
        return self._plin(mlp.fc_out, self._plin(mlp.fc_in, x, act))

    # ------------------------------------------------------------- prefill
    @torch.no_grad()
    def prefill(self, ids: torch.Tensor, slots: list[int], lens: list[int] | None = None,
                start: list[int] | None = None) -> torch.Tensor:
        """ids [n, T] prompts, right-padded to T when ``lens`` (their true
        lengths) is given -> last-real-position logits [n, V]. Writes K/V of
        positions [0, lens[i]) into each slot and marks the prompt as seen.
        Padding needs no mask: with causal attention a real query row never
        sees a key to its right, so ragged prompts batch into one pass.

        ``start`` (chunked prefill): row i continues slot i's sequence at
        position start[i] -- its K/V land at [start, start + lens[i]) and its
        queries attend to the cached prefix plus the chunk."""
        m, cfg = self.model, self.cfg
        ids = ids.to(self.device)
        n, T = ids.shape
        lens = [T] * n if lens is None else [int(x) for x in lens]
        start = [0] * n if start is None else [int(x) for x in start]
        assert len(lens) == n and len(start) == n and all(0 < L <= T for L in lens)
        assert all(p0 + L <= self.max_len for p0, L in zip(start, lens))
        ragged = any(L != T for L in lens)
        cont = any(start)
        for s_, L, p0 in zip(slots, lens, start):
            if p0 == 0:
                self.cache.release(s_)  # a reused slot starts empty
            self.cache.reserve(s_, p0 + L)
        self.cache.sync()
        plan = self.cache.plan_write(slots, lens, T, start)
        sl = torch.tensor(slots, device=self.device, dtype=torch.long)
        fresh = [i for i, p0 in enumerate(start) if p0 == 0]
        if len(fresh) == n:
            self.seen[sl] = 0
        elif fresh:
            self.seen[sl[fresh]] = 0
        if ragged:
            valid = torch.arange(T, device=self.device)[None] < torch.tensor(lens, device=self.device)[:, None]
            self.seen[sl[:, None].expand(n, T)[valid], ids[valid]] = 1
        else:
            self.seen[sl[:, None].expand(n, T), ids] = 1
        pos_ids = None
        if cont:
            pos_ids = (torch.tensor(start, device=self.device)[:, None]
                       + torch.arange(T, device=self.device)[None]).clamp_(max=self.max_len - 1)
        h = m.embed(ids, pos_ids if cont else None)
        pending = ()
        rows_d = None
        for li, blk in enumerate(m.h):
            if self.multi_device and h.device != self.layer_devs[li]:
                h, pending = self._hop(self.layer_devs[li], h, pending)
            x, h = blk.ln_1(h, residual=pending) if pending else (blk.ln_1(h), h)
            at = blk.attn
            qkv = self._plin(at.qkv, x).view(n, T, 3, self.H, self.D)
            q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            if self.rot > 0:
                ops.apply_rotary_(q, k, self.rot, T, cfg.rotary_interleaved, cfg.rotary_base,
                                  pos_ids=pos_ids, max_pos=self.max_len)
            self.cache.write(li, k, v, slots, lens, plan, start)
            if cont and self.prefix_cache and self._paged_prefill(at, n, T, start):
                if rows_d is None:  # one upload per prefill: the rows' slots, first positions and lengths
                    rows_d = torch.tensor([slots, start, lens], dtype=torch.int32).to(self.device)
                o = prefill_paged.prefill_paged_attention(q, self.cache.k[li], self.cache.v[li], rows_d[0], rows_d[1],
                                                          rows_d[2], at.scale, at.alibi,
                                                          block_table=self.cache.table_on(self.layer_devs[li]))
                self.paged_prefill_calls += 1
            elif cont:
                self.gather_prefill_calls += 1
                o = self._continued_attention(li, q, slots, lens, start, at, cur=(k, v))
            else:  # (GPT-Neo local layers: banded, the kernels skip the tiles left of the band)
                o = ops.flash_attention(q, k, v, causal=True, scale=at.scale, alibi=at.alibi, window=at.window)
            a = self._plin(at.out, o.reshape(n, T, -1))
            if cfg.parallel_residual:
                x2 = x if blk.ln_2 is None else blk.ln_2(h)
                pending = (a, self._pmlp(blk.mlp, x2))
            else:
                x2, h = blk.ln_2(h, residual=(a,))
                pending = (self._pmlp(blk.mlp, x2),)
        if self.multi_device and h.device != self.head_dev:
            h, pending = self._hop(self.head_dev, h, pending)
        if ragged:
            rows = torch.arange(n, device=h.device)
            last = torch.tensor(lens, device=h.device) - 1
            pick = lambda t: t[rows, last][:, None]  # noqa: E731
        else:
            pick = lambda t: t[:, -1:]  # noqa: E731
        y, _ = m.ln_f(pick(h), residual=tuple(pick(p_) for p_ in pending))
        return m.logits_from_hidden(y)[:, -1].to(self.device)

    def _paged_prefill(self, at, n: int, T: int, start: list[int]) -> bool:
        """Whether a continued prefill's attention runs ``kca_prefill_paged_attn``: where the kernel covers
        the layer, except ONE bf16 row of >= 512 queries behind >= 2048 cached tokens, the one cell of
        bench/prefix_bench.py where the gather loop measured faster by more than the spread (NeoX heads:
        0.149 against 0.159 ms; one row is 4 query tiles x H workgroups, and the gathered copy takes
        flash attention's full-tile path; docs/PERF.md, Round 14). fp16 always runs the kernel: the gather
        loop's flash attention is not native for it."""
        if not prefill_paged.supported(self.D, self.H, self.Hkv, at.window):
            return False
        return not (n == 1 and T >= 512 and start[0] >= 2048 and self.dtype == torch.bfloat16
                    and self.device.type == "cuda")

    def _continued_attention(self, li, q, slots, lens, start, at, cur=None):
        """Chunk queries [start, start + L) of each row against the slot's cached
        keys [0, start + L) (just written): bottom-right-aligned causal mask,
        so query j of the chunk sees keys <= start + j. FP8 KV cache: the gathered window is
        dequantized to the model dtype, so the earlier chunks are seen as stored (quantized) and the
        current chunk exact (its own 16-bit K / V, not what was just written)."""
        n, T = q.shape[0], q.shape[1]
        o = torch.zeros_like(q)
        kc, vc, tbl = self.cache.k[li], self.cache.v[li], self.cache.table_on(self.layer_devs[li])
        for i, (s_, L, p0) in enumerate(zip(slots, lens, start)):
            kv = p0 + L
            lo = max(0, kv - L - at.window + 1) if at.window else 0  # oldest key any chunk query can see
            if self._kv8:
                ksc, vsc = self.cache.k_scale[li], self.cache.v_scale[li]
                kw, vw = cur[0][i, :L], cur[1][i, :L]
                if p0 > 0:
                    kw = torch.cat((kv8.gather_kv8(kc, ksc, s_, p0, tbl, q.dtype).transpose(0, 1), kw))
                    vw = torch.cat((kv8.gather_kv8(vc, vsc, s_, p0, tbl, q.dtype).transpose(0, 1), vw))
                kw, vw = kw[lo:][None], vw[lo:][None]
            else:
                kw = dops.gather_kv(kc, s_, kv, tbl)[:, lo:].transpose(0, 1)[None]
                vw = dops.gather_kv(vc, s_, kv, tbl)[:, lo:].transpose(0, 1)[None]
            o[i:i + 1, :L] = ops.flash_attention(q[i:i + 1, :L], kw, vw, causal=True, scale=at.scale,
                                                 alibi=at.alibi, window=at.window)
        return o

    @staticmethod
    def _hop(dev, h, pending):
        """Move the residual stream to the next layer-split device."""
        return h.to(dev), tuple(p_.to(dev) for p_ in pending)

    # -------------------------------------------------------------- decode
    def _fused_bufs(self):
        """Static buffers of the fused batch-1 layer (allocated outside any graph capture)."""
        fz = self._fz.get("b1")
        if fz is None:
            d, f = self.cfg.hidden, self.model.h[0].mlp.fc_in.weight.shape[0]
            z = dict(device=self.device, dtype=self.dtype)
            biases = []
            for blk in self.model.h:
                bo, bf = blk.attn.out.bias, blk.mlp.fc_out.bias
                biases.append(bf if bo is None else (bo if bf is None else (bo.float() + bf.float()).to(self.dtype)))
            fz = self._fz["b1"] = {
                "g": torch.empty(1, f, **z), "h": torch.empty(1, d, **z), "xn": torch.empty(1, d, **z),
                "xn2": torch.empty(1, d, **z), "ypart": torch.empty(d, device=self.device, dtype=torch.float32),
                "cnt": torch.zeros(32 * 65, device=self.device, dtype=torch.int32), "bias": biases}
        return fz

    def _desc_args(self, cos, sin, tbl):
        """(cos, sin, block table, by_row) for the decode attention: the step descriptors' rows where
        this step has them (see _STEP_DESC), else the position tables and the device block table."""
        by_row = 0
        if self._step_desc is not None:
            rc, rs, pages = self._step_desc
            if rc is not None and cos is not None:
                cos, sin, by_row = rc, rs, 1
            if pages is not None and tbl is not None:
                tbl, by_row = pages, by_row | 2
        return cos, sin, tbl, by_row

    def _attn(self, qkv, at, kc, vc, cos, sin, pos, slots, kv_lens, max_kv, obuf, ws, tbl, by_row):
        """A layer's RoPE + cache append + attention for the step being built: one token per row
        (``decode_prep_attention``), or -- while a verify step is built -- T rows per sequence
        (``spec_prep_attention``, whose per-sequence arrays ``verify_async`` left in ``_spec``)."""
        cfg = self.cfg
        if self._spec is not None:
            base, n_tok, sl, kl, T, rows = self._spec
            assert not by_row, "a verify step looks its angles and pages up on the device"
            if rows is not None:  # a short KV stream: the rows as sequences of their own (_spec_rows)
                spec.spec_prep(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved, cos, sin, base, n_tok,
                               sl, T, kc, vc, tbl)
                return dops.decode_attention(qkv, kc, vc, rows[0], rows[1], self.H, max_kv, at.scale, at.alibi,
                                             out=obuf, ws=ws, block_table=tbl, window=at.window)
            return spec.spec_prep_attention(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved, cos, sin,
                                            base, n_tok, sl, T, kc, vc, kl, max_kv, at.scale, at.alibi, out=obuf,
                                            ws=ws, block_table=tbl, window=at.window)
        return dops.decode_prep_attention(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved,
                                          cos, sin, pos, slots, kc, vc, kv_lens, max_kv, at.scale, at.alibi,
                                          out=obuf, ws=ws, block_table=tbl, window=at.window, by_row=by_row)

    def _layers_decode_fused(self, tokens, pos, slots, kv_lens, max_kv, ws, obuf):
        """Batch-1 decode step, one queue, the residual + next LayerNorm in each layer's last projection
        (see _fused_ok for the three layer kinds). Returns None (nothing launched) when the fused kernels
        do not cover the shape."""
        m, cfg = self.model, self.cfg
        fz = self._fused_bufs()
        kind = self._layer_kind
        blk0 = m.h[0]
        if self._embed_head:  # token gather (+ chained token) + LayerNorm: one kernel
            chain, prev = self._chain_src if self._chain_src is not None else (None, None)
            if m.emb_ln is not None:  # BLOOM: the residual stream starts at LN_emb(wte[id])
                h, _ = embed_ln_rows(m.wte.weight, tokens, m.emb_ln.weight, m.emb_ln.bias, m.emb_ln.eps,
                                     chain=chain, prev=prev)
                xn, _ = ln_rows(h, blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps)
            else:
                xn, h = embed_ln_rows(m.wte.weight, tokens, blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps,
                                      chain=chain, prev=prev)
        else:
            h0 = m.embed(tokens, pos.long())
            xn, h = ln_rows(h0, blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps)
        xn2 = ln_rows(h, blk0.ln_2.weight, blk0.ln_2.bias, blk0.ln_2.eps)[0] if kind == "neox" else None
        hb, xb, x2b, g = fz["h"], fz["xn"], fz["xn2"], fz["g"]
        tbl = self.cache.table_on(self.device)
        cos, sin, tbl, by_row = self._desc_args(self.cos, self.sin, tbl)
        for li, blk in enumerate(m.h):
            at, mlp = blk.attn, blk.mlp
            act = 1 if mlp.approx in ("tanh", True) else 2
            kc, vc = self.cache.k[li], self.cache.v[li]
            nxt = m.h[li + 1] if li + 1 < len(m.h) else None
            nln = nxt.ln_1 if nxt is not None else m.ln_f
            qkv = skinny_linear(xn, at.qkv.weight, at.qkv.bias)
            if kind == "seq" and self._tp_ar is not None:
                # TP rank: partial projections, each closed by all-reduce + bias + residual + LayerNorm
                ar = self._tp_ar
                o = dops.decode_prep_attention(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved,
                                               cos, sin, pos, slots, kc, vc, kv_lens, max_kv, at.scale, at.alibi,
                                               out=obuf, ws=ws, block_table=tbl, window=at.window, by_row=by_row)
                ar.res_ln(skinny_linear(o, at.out.weight), at.out.bias, h, hb, blk.ln_2.weight, blk.ln_2.bias,
                          blk.ln_2.eps, x2b)
                f = skinny_linear(x2b, mlp.fc_in.weight, mlp.fc_in.bias, act, out=g)
                ar.res_ln(skinny_linear(f, mlp.fc_out.weight), mlp.fc_out.bias, hb, hb, nln.weight, nln.bias,
                          nln.eps, xb)
                h, xn = hb, xb
                continue
            if kind == "seq":
                # attention, out-projection + residual + ln_2, fc_in (+ GELU), fc_out + residual + next ln_1
                # (a fused attention + out-projection launch and tail launches chained with the next
                # projection measured slower: profiles/decode_launch_structure_ab_r5.txt)
                o = dops.decode_prep_attention(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved,
                                               cos, sin, pos, slots, kc, vc, kv_lens, max_kv, at.scale, at.alibi,
                                               out=obuf, ws=ws, block_table=tbl, window=at.window, by_row=by_row)
                dops.gemv_dual_ln(o, at.out.weight, None, None, at.out.bias, h, blk.ln_2.weight, blk.ln_2.bias,
                                  blk.ln_2.eps, fz["ypart"], fz["cnt"], hb, x2b)
                f = skinny_linear(x2b, mlp.fc_in.weight, mlp.fc_in.bias, act, out=g)
                dops.gemv_dual_ln(f, mlp.fc_out.weight, None, None, mlp.fc_out.bias, hb, nln.weight, nln.bias,
                                  nln.eps, fz["ypart"], fz["cnt"], hb, xb)
                h, xn = hb, xb
                continue
            # parallel residual: attention + fc_in (of ln_2's output for NeoX) in one launch
            if not dops.decode_prep_attention_gemv(
                    qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved, cos, sin, pos, slots, kc, vc,
                    kv_lens, max_kv, at.scale, at.alibi, obuf, ws, tbl, at.window,
                    xn2 if kind == "neox" else xn, mlp.fc_in.weight, mlp.fc_in.bias, g, act, by_row):
                if li == 0:
                    return None
                raise RuntimeError("fused decode layer: shape support changed between layers")
            two = kind == "neox" and nxt is not None
            dops.gemv_dual_ln(obuf, at.out.weight, g, mlp.fc_out.weight, fz["bias"][li], h, nln.weight, nln.bias,
                              nln.eps, fz["ypart"], fz["cnt"], hb, xb,
                              *((nxt.ln_2.weight, nxt.ln_2.bias, x2b) if two else ()))
            h, xn, xn2 = hb, xb, (x2b if two else None)
        if m.lm_head is None:
            return skinny_linear(xn, m.wte.weight)
        return self._lin(m.lm_head, xn)

    def _batched_bufs(self, B: int):
        """Static buffers of the batched matrix-core layer for a batch bucket (outside graph capture)."""
        key = ("mm", B)
        fz = self._fz.get(key)
        if fz is None:
            m = self.model
            d = self.cfg.hidden
            at0, mlp0 = m.h[0].attn, m.h[0].mlp
            z = dict(device=self.device, dtype=self.dtype)
            biases = []
            for blk in m.h:
                bo, bf = blk.attn.out.bias, blk.mlp.fc_out.bias
                biases.append(bf if bo is None else (bo if bf is None else (bo.float() + bf.float()).to(self.dtype)))
            fz = self._fz[key] = {
                "h": torch.empty(B, d, **z), "xn": torch.empty(B, d, **z), "xn2": torch.empty(B, d, **z),
                "qkv": torch.empty(B, at0.qkv.weight.shape[0], **z), "g": torch.empty(B, mlp0.fc_in.weight.shape[0], **z),
                "y": torch.empty(B, d, **z),  # a TP rank's partial projection before the all-reduce
                "st": smm.RowStatsBuf(B, d, self.device), "bias": biases}
        return fz

    def _head_weight(self):
        from ..parallel.tensor_parallel import ParallelLMHead
        m = self.model
        if m.lm_head is None:
            return m.wte.weight, None, None
        if isinstance(m.lm_head, ParallelLMHead):
            return m.lm_head.local_weight(), m.lm_head.bias, m.lm_head.group
        return m.lm_head.weight, m.lm_head.bias, None

    def _layers_decode_batched(self, tokens, pos, slots, kv_lens, max_kv, ws, obuf):
        """Decode step at batch 2..64 on the matrix cores (see _batched_ok). Per layer kind:
          seq  : QKV(LN1 on load) -> attention -> out + b + h (stats) -> fc_in(LN2 on load, GELU) -> fc_out + b + h
          gptj : [QKV | fc_in+GELU](LN1 on load) -> attention -> o.Wo + g.Wf + b + h (stats)
          neox : as gptj, fc_in normalising with ln_2's gamma / beta (same statistics)
        Layer 0 reads the step head's normalised rows; the LM head normalises with ln_f on load."""
        m, cfg = self.model, self.cfg
        B = tokens.shape[0]
        fz = self._batched_bufs(B)
        self.batched_steps += 1  # (counted when a step is built: eager runs and graph captures)
        kind = self._layer_kind
        blk0 = m.h[0]
        hb, st, qkv, g = fz["h"], fz["st"], fz["qkv"], fz["g"]
        dt = self.dtype
        # step head: token rows (+ BLOOM's embedding LayerNorm) and ln_1 (+ ln_2 for NeoX) of layer 0
        if self._embed_head:  # (resolves a chained token of the previous step on the device, as at B = 1)
            chain, prev = self._chain_src if self._chain_src is not None else (None, None)
            if m.emb_ln is not None:
                h, _ = embed_ln_rows(m.wte.weight, tokens, m.emb_ln.weight, m.emb_ln.bias, m.emb_ln.eps,
                                     chain=chain, prev=prev)
                xn, h = ln_rows(h, blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps)
            else:
                xn, h = embed_ln_rows(m.wte.weight, tokens, blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps,
                                      chain=chain, prev=prev)
        else:
            xn, h = ln_rows(m.embed(tokens, pos.long()), blk0.ln_1.weight, blk0.ln_1.bias, blk0.ln_1.eps)
        xn2 = ln_rows(h, blk0.ln_2.weight, blk0.ln_2.bias, blk0.ln_2.eps)[0] if kind == "neox" else None
        hb.copy_(h)
        tbl = self.cache.table_on(self.device)
        cos, sin, tbl, by_row = self._desc_args(self.cos, self.sin, tbl)
        pk = self._packed_w

        def part(x, w, ln=None):  # one K-part, streaming the weight's packed twin
            return smm.part(x, w, ln, packed=pk(w))

        for li, blk in enumerate(m.h):
            at, mlp = blk.attn, blk.mlp
            act = 1 if mlp.approx in ("tanh", True) else 2
            nxt = m.h[li + 1] if li + 1 < len(m.h) else None
            nln = nxt.ln_1 if nxt is not None else m.ln_f
            first = li == 0
            ln1 = None if first else (st, blk.ln_1.weight, blk.ln_1.bias)
            x1 = xn if first else hb
            kc, vc = self.cache.k[li], self.cache.v[li]
            if kind == "seq" and self._tp_ar is not None:
                # TP rank: partial projections, each closed by all-reduce + bias + residual + row statistics
                ar, y = self._tp_ar, fz["y"]
                smm.launch([smm.job([part(x1, at.qkv.weight, ln1)], qkv.shape[1], qkv, at.qkv.bias)], B, dt)
                o = self._attn(qkv, at, kc, vc, cos, sin, pos, slots, kv_lens, max_kv, obuf, ws, tbl, by_row)
                smm.mm(o, at.out.weight, out=y, packed=pk(at.out.weight))
                ar.res_stats(y, at.out.bias, hb, hb, st, blk.ln_2.eps)
                smm.launch([smm.job([part(hb, mlp.fc_in.weight, (st, blk.ln_2.weight, blk.ln_2.bias))],
                                    g.shape[1], g, mlp.fc_in.bias, act)], B, dt)
                smm.mm(g, mlp.fc_out.weight, out=y, packed=pk(mlp.fc_out.weight))
                ar.res_stats(y, mlp.fc_out.bias, hb, hb, st, nln.eps)
                continue
            if kind == "seq":
                smm.launch([smm.job([part(x1, at.qkv.weight, ln1)], qkv.shape[1], qkv, at.qkv.bias)], B, dt)
                o = self._attn(qkv, at, kc, vc, cos, sin, pos, slots, kv_lens, max_kv, obuf, ws, tbl, by_row)
                smm.launch([smm.job([part(o, at.out.weight)], hb.shape[1], hb, at.out.bias, res=hb, stats=st,
                                    eps=blk.ln_2.eps)], B, dt)
                smm.launch([smm.job([part(hb, mlp.fc_in.weight, (st, blk.ln_2.weight, blk.ln_2.bias))],
                                    g.shape[1], g, mlp.fc_in.bias, act)], B, dt)
                smm.launch([smm.job([part(g, mlp.fc_out.weight)], hb.shape[1], hb, mlp.fc_out.bias, res=hb,
                                    stats=st, eps=nln.eps)], B, dt)
                continue
            # parallel residual: [QKV | fc_in] of the same residual rows, one launch
            if kind == "neox":
                ln2 = (st, blk.ln_2.weight, blk.ln_2.bias) if not first else None
                x2 = xn2 if first else hb
            else:
                ln2, x2 = ln1, x1
            smm.launch([smm.job([part(x1, at.qkv.weight, ln1)], qkv.shape[1], qkv, at.qkv.bias),
                        smm.job([part(x2, mlp.fc_in.weight, ln2)], g.shape[1], g, mlp.fc_in.bias, act)], B, dt)
            o = self._attn(qkv, at, kc, vc, cos, sin, pos, slots, kv_lens, max_kv, obuf, ws, tbl, by_row)
            smm.launch([smm.job([part(o, at.out.weight), part(g, mlp.fc_out.weight)], hb.shape[1], hb,
                                fz["bias"][li], res=hb, stats=st, eps=nln.eps)], B, dt)
        w, b, grp = self._head_weight()
        V = w.shape[0]
        if V % 4 == 0:
            logits = smm.mm(hb, w, b, ln=(st, m.ln_f.weight, m.ln_f.bias), packed=pk(w))
        else:  # (GPT-2's 50257 rows: the head takes the normalised rows through the plain path)
            y = smm.ln_on_load_reference(hb, st.merged(hb.shape[0]), m.ln_f.weight, m.ln_f.bias)
            logits = skinny_linear(y, w, b)
        if grp is not None:
            from ..parallel.tensor_parallel import gather_last_dim
            logits = gather_last_dim(logits, grp)
        return logits

    def _packed_w(self, w):
        """The packed stream twin of a weight the matrix-core layer reads (``skinny_mm.pack_weight``):
        built once, on the first (eager) step that uses it -- the graph-capture warm-up -- and kept for the
        runner's life (KCA_MM_PACK=0: none, the row-major weight streams). Keyed by storage address,
        shape and version (an in-place weight update re-packs)."""
        if not smm.PACK:
            return None
        key = (w.data_ptr(), tuple(w.shape), w._version)
        p = self._packs.get(key)
        if p is None and not torch.cuda.is_current_stream_capturing():
            p = self._packs[key] = smm.pack_weight(w.detach())
        return p

    def _layers_decode(self, tokens, pos, slots, kv_lens, max_kv, ws, obuf):
        m, cfg = self.model, self.cfg
        w8 = self._w8 is not None  # FP8 weights: the per-projection path at every batch size
        self.w8_steps += w8
        self.mx4_steps += self._mx4 is not None
        self.kv8_steps += self._kv8
        w8 = w8 or self._mx4 is not None or self._kv8  # MXFP4 weights likewise; FP8 KV cache: the per-projection path too (its attention is its own launches)
        if not w8 and self._fused_ok and tokens.shape[0] == 1 and obuf is not None:
            y = self._layers_decode_fused(tokens, pos, slots, kv_lens, max_kv, ws, obuf)
            if y is not None:
                self.fused_steps += 1
                return y
        if (not w8 and self._batched_ok and 2 <= tokens.shape[0] <= min(smm.MAX_M, self._batched_max_b)
                and obuf is not None
                and (self._chain_src is None or self._embed_head)):
            return self._layers_decode_batched(tokens, pos, slots, kv_lens, max_kv, ws, obuf)
        if self._chain_src is not None and obuf is not None:  # chained rows not resolved by a fused head
            chain, prev = self._chain_src
            tokens = torch.where(chain[:tokens.shape[0]] >= 0, prev[chain[:tokens.shape[0]].clamp(min=0).long()],
                                 tokens)
        h = m.embed(tokens, pos.long())
        pending = ()
        per_dev = {self.device: (pos, slots, kv_lens, ws, obuf)}
        for li, blk in enumerate(m.h):
            # every LayerNorm (+ pending residual adds) runs as the prologue of the GEMM that consumes it
            at = blk.attn
            dev = self.layer_devs[li]
            if self.multi_device:
                if h.device != dev:
                    h, pending = self._hop(dev, h, pending)
                if dev not in per_dev:
                    per_dev[dev] = (pos.to(dev), slots.to(dev), kv_lens.to(dev), None, None)
                pos, slots, kv_lens, ws, obuf = per_dev[dev]
            shared = cfg.parallel_residual and blk.ln_2 is None  # GPT-J: one LN feeds qkv and fc_in
            # (forking before the QKV GEMV was measured slower at B=1, 3.09 vs 2.99 ms on one box: the
            # QKV GEMV then shares HBM with the MLP GEMVs and the attention chain starts later)
            if shared:
                qkv, h, xn = self._ln_lin(blk.ln_1, h, pending, at.qkv, want_xn=True)
            else:
                qkv, h = self._ln_lin(blk.ln_1, h, pending, at.qkv)
            mlp = blk.mlp
            act = 1 if mlp.approx in ("tanh", True) else 2
            side_out = None
            if self._par_mlp:  # fork: MLP branch on the side stream
                cur = torch.cuda.current_stream()
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side):
                    if shared:
                        xm = xn
                    else:
                        xm, _ = self._ln_lin(blk.ln_2, h, (), mlp.fc_in, act)  # NeoX: ln_2 + fc_in fused
                    side_out = self._lin(mlp.fc_out, self._lin(mlp.fc_in, xm, act) if shared else xm)
                if not torch.cuda.is_current_stream_capturing():  # eager: keep cross-stream buffers alive
                    xm.record_stream(self._side)
                    h.record_stream(self._side)
            kc, vc, tbl = self.cache.k[li], self.cache.v[li], self.cache.table_on(dev)
            cos, sin = self._rope[dev]
            by_row = 0
            if obuf is not None and not self.multi_device and not self._kv8:  # a graph-bucket step: its descriptors
                cos, sin, tbl, by_row = self._desc_args(cos, sin, tbl)
            # RoPE + cache append + split-K attention (one launch on the GPU; GPT-Neo local layers read
            # only the last `window` positions)
            if self._kv8:  # FP8 KV cache: quantizing prep, attention over the bytes (+ combine past one split)
                o = kv8.kv8_prep_attention(qkv, self.H, self.Hkv, self.D, self.rot, cfg.rotary_interleaved,
                                           cos, sin, pos, slots, kc, vc, self.cache.k_scale[li],
                                           self.cache.v_scale[li], kv_lens, max_kv, at.scale, at.alibi,
                                           out=obuf, ws=ws, block_table=tbl, window=at.window)
            else:
                o = self._attn(qkv, at, kc, vc, cos, sin, pos, slots, kv_lens, max_kv, obuf, ws, tbl, by_row)
            a = self._lin(at.out, o)
            if side_out is not None:  # join
                cur.wait_stream(self._side)
                if not torch.cuda.is_current_stream_capturing():
                    side_out.record_stream(cur)
                pending = (a, side_out)
            elif shared:
                pending = (a, self._lin(mlp.fc_out, self._lin(mlp.fc_in, xn, act)))
            elif cfg.parallel_residual:
                f, _ = self._ln_lin(blk.ln_2, h, (), mlp.fc_in, act)
                pending = (a, self._lin(mlp.fc_out, f))
            else:
                f, h = self._ln_lin(blk.ln_2, h, (a,), mlp.fc_in, act)
                pending = (self._lin(mlp.fc_out, f),)
        if self.multi_device and h.device != self.head_dev:
            h, pending = self._hop(self.head_dev, h, pending)
        if m.lm_head is None:
            y = self._ln_lin(m.ln_f, h, pending, None, weight=m.wte.weight)[0]
        else:
            y = self._ln_lin(m.ln_f, h, pending, m.lm_head)[0]
        return y.to(self.device) if self.multi_device else y

    def _ln_lin(self, ln, h, res, mod, act: int = 0, weight=None, want_xn: bool = False):
        """LayerNorm(h + sum(res)) -> column-parallel / LM-head linear, fused (decode)."""
        from ..parallel.tensor_parallel import ParallelLMHead, RowParallelLinear, gather_last_dim
        assert not isinstance(mod, RowParallelLinear)
        if self._w8 is not None and id(mod) in self._w8:  # FP8 weights: LayerNorm rows, then the e4m3 stream
            xn, h = ln_rows(h, ln.weight, ln.bias, ln.eps, res)
            y = w8_linear(xn, self._w8[id(mod)], mod.bias, act)
            return (y, h, xn) if want_xn else (y, h)
        if self._mx4 is not None and id(mod) in self._mx4:  # MXFP4 weights: the same, on the nibble stream
            xn, h = ln_rows(h, ln.weight, ln.bias, ln.eps, res)
            y = mx4.mx4_linear(xn, self._mx4[id(mod)], mod.bias, act)
            return (y, h, xn) if want_xn else (y, h)
        if isinstance(mod, ParallelLMHead):
            y, h = ln_skinny_linear(h, ln.weight, ln.bias, ln.eps, mod.local_weight(), mod.bias, res, act)
            return gather_last_dim(y, mod.group), h
        return ln_skinny_linear(h, ln.weight, ln.bias, ln.eps, mod.weight if weight is None else weight,
                                None if mod is None else mod.bias, res, act, want_xn=want_xn)

    # decode linears: skinny GEMM (W streamed once, bias/GELU fused) for <= 16 rows
    def _lin(self, mod, x, act: int = 0):
        from ..parallel.tensor_parallel import ParallelLMHead, RowParallelLinear, gather_last_dim, reduce_from_tp
        if self._w8 is not None and id(mod) in self._w8:
            return w8_linear(x, self._w8[id(mod)], mod.bias, act)
        if self._mx4 is not None and id(mod) in self._mx4:
            return mx4.mx4_linear(x, self._mx4[id(mod)], mod.bias, act)
        if isinstance(mod, RowParallelLinear):
            y = reduce_from_tp(skinny_linear(x, mod.weight, None), mod.group)
            return y + mod.bias if mod.bias is not None else y
        if isinstance(mod, ParallelLMHead):
            return gather_last_dim(skinny_linear(x, mod.local_weight(), mod.bias), mod.group)
        return skinny_linear(x, mod.weight, mod.bias, act)

    def _static_for(self, Bb: int, Kb: int):
        key = (Bb, Kb)
        st = self._static.get(key)
        if st is not None:
            return st
        NB = self.max_bans
        pk = _Packed({"tokens": (torch.int64, Bb), "seeds": (torch.int64, Bb), "pos": (torch.int32, Bb),
                      "slots": (torch.int32, Bb), "kv_lens": (torch.int32, Bb), "top_k": (torch.int32, Bb),
                      "temperature": (torch.float32, Bb), "top_p": (torch.float32, Bb),
                      "rep": (torch.float32, Bb), "bans": (torch.int32, Bb * NB),
                      "chain": (torch.int32, Bb), **self._desc_fields(Bb)}, self.device)
        ws_n = dops.decode_ws_floats(Bb, self.H, self.Hkv, self.D, Kb)
        ob = self._outbuf(Bb)
        st = {
            "pk": pk,
            "ws": torch.zeros(max(ws_n, 1), device=self.device, dtype=torch.float32),  # zeroed: fan-in counters
            "obuf": torch.empty(Bb, self.H * self.D, device=self.device, dtype=self.dtype),
            "sws": torch.empty(Bb * self.V, device=self.device, dtype=torch.float32),
            **ob,
        }
        self._static[key] = st
        return st

    def _desc_on(self, Bb: int) -> bool:
        return (_STEP_DESC and (Bb == 1 or _STEP_DESC_BATCHED) and self.device.type == "cuda"
                and not self.multi_device and (self.rot > 0 or self.cache.paged))

    def _desc_fields(self, Bb: int) -> dict:
        """Per-step descriptor arrays (see _STEP_DESC): row i's RoPE angles and page-table row."""
        if not self._desc_on(Bb):
            return {}
        f = {}
        if self.rot > 0:
            f["rcos"] = (torch.float32, Bb * (self.rot // 2))
            f["rsin"] = (torch.float32, Bb * (self.rot // 2))
        if self.cache.paged:
            f["pages"] = (torch.int32, Bb * self.cache.blocks)
        return f

    def _fill_desc(self, a, Bb: int, pos, slots):
        """Host side of the step descriptors: row i's RoPE angles at its position and its page row."""
        if "rcos" in a:
            half = self.rot // 2
            ch, sh = self._rope_h
            a["rcos"].reshape(Bb, half)[:] = ch[pos[:Bb]]
            a["rsin"].reshape(Bb, half)[:] = sh[pos[:Bb]]
        if "pages" in a:
            a["pages"].reshape(Bb, self.cache.blocks)[:] = self.cache.table_h.numpy()[slots[:Bb]]

    def _desc_views(self, pk, Bb: int):
        """(cos rows, sin rows, page rows) device views of the step descriptors (None where absent)."""
        f = pk.fields
        return (pk.d("rcos") if "rcos" in f else None, pk.d("rsin") if "rsin" in f else None,
                pk.d("pages").view(Bb, self.cache.blocks) if "pages" in f else None)

    def _outbuf(self, Bb: int, key=None):
        """Sampled ids (int64) and log-probs (fp32) of a batch bucket in ONE device buffer shared by its
        kv-length buckets -- one D2H copy per step, and a chained token (decode_async) is read by the
        next step's embedding kernel from a fixed address whatever kv bucket that step lands in --
        with two pinned landing buffers (one per host pk buffer)."""
        key = Bb if key is None else key  # (a verify bucket keeps its own: key ("spec", rows))
        ob = self._outbufs.get(key)
        if ob is None:
            pin = self.device.type == "cuda"
            dev = torch.empty(3 * Bb, device=self.device, dtype=torch.int32)
            hs = [torch.empty(3 * Bb, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
            # "flip": the landing buffer of the latest launch, counted per BATCH bucket (every kv bucket of
            # this Bb copies into these two buffers, so consecutive launches must alternate here even when
            # they land in different kv buckets -- a per-(Bb, Kb) counter could hand two in-flight steps
            # the same buffer)
            ob = {"out": dev, "ids": dev[:2 * Bb].view(torch.int64), "lps": dev[2 * Bb:].view(torch.float32),
                  "flip": [0], "out_h": hs, "ids_h": [h[:2 * Bb].view(torch.int64) for h in hs],
                  "lps_h": [h[2 * Bb:].view(torch.float32) for h in hs]}
            self._outbufs[key] = ob
        return ob

    def _step_body(self, st, Bb, Kb, mc=False):
        n0 = _lib.LAUNCHES[0]
        try:
            self._step_body_inner(st, Bb, Kb, mc)
        finally:
            # native launches one decode step issues (counted when the step is built: eager, or graph capture)
            self.step_launches[Bb] = _lib.LAUNCHES[0] - n0

    def _step_body_inner(self, st, Bb, Kb, mc=False):
        pk = st["pk"]
        # chained tokens resolved on the device by the fused B = 1 step head (_layers_decode_fused)
        self._chain_src = (pk.d("chain"), st["ids"]) if (Bb == 1 and self._embed_head) else None
        if "rcos" in pk.fields or "pages" in pk.fields:
            self._step_desc = self._desc_views(pk, Bb)
        try:
            logits = self._layers_decode(pk.d("tokens"), pk.d("pos"), pk.d("slots"), pk.d("kv_lens"), Kb,
                                         st["ws"], st["obuf"])
        finally:
            self._step_desc = None
        dops.sample_logits(logits, temperature=pk.d("temperature"), top_k=pk.d("top_k"), top_p=pk.d("top_p"),
                           rep_penalty=pk.d("rep"), seen=self.seen, slots=pk.d("slots"),
                           ban_ids=pk.d("bans").view(Bb, self.max_bans), seeds=pk.d("seeds"), step=0,
                           ws=st["sws"], out_ids=st["ids"], out_logprobs=st["lps"], mwg_complete=mc)

    # ----------------------------------------------------------- beam search
    @torch.no_grad()
    def decode_topk(self, tokens: list[int], positions: list[int], slots: list[int], k: int):
        """Eager decode step returning the top-k next-token log-probs per row
        (beam search; K30). -> (logprobs [n, k] fp32, ids [n, k] int64) on device."""
        dev = self.device
        for s_, p_ in zip(slots, positions):
            self.cache.reserve(s_, p_ + 1)
        self.cache.sync()
        tok = torch.tensor(tokens, device=dev, dtype=torch.long)
        pos = torch.tensor(positions, device=dev, dtype=torch.int32)
        sl = torch.tensor(slots, device=dev, dtype=torch.int32)
        kl = pos + 1
        max_kv = max(positions) + 1
        logits = self._layers_decode(tok, pos, sl, kl, max_kv, None, None)
        lp = torch.log_softmax(logits.float(), dim=-1)
        return lp.topk(k, dim=-1)

    @torch.no_grad()
    def copy_slots(self, dst: list[int], src: list[int], upto: int):
        """KV cache (and seen mask) of ``src`` slots -> ``dst`` slots, positions
        [0, upto) (paged: prefix pages shared, see ``KVCache.fork``)."""
        if not dst:
            return
        self.cache.fork(dst, src, upto)
        self.cache.sync()
        d = torch.tensor(dst, device=self.device, dtype=torch.long)
        s = torch.tensor(src, device=self.device, dtype=torch.long)
        self.seen[d] = self.seen[s]

    def release(self, slot: int):
        """A finished sequence's KV pages go back to the pool."""
        self.cache.release(slot)

    @torch.no_grad()
    def adopt_prefix(self, slot: int, pages: list[int], tokens: list[int]):
        """Prefix caching: ``pages`` (a ``KVCache.lookup`` chain holding the K/V of ``tokens``) become the
        first pages of ``slot``, shared, and ``tokens`` its seen set -- the repetition penalty sees the
        cached prefix. ``prefill(..., start=[len(tokens)])`` continues from there (it resets neither)."""
        if not self.prefix_cache:
            raise ValueError("adopt_prefix needs prefix_cache=True (KCA_PREFIX_CACHE=1)")
        assert len(tokens) == len(pages) * self.cache.page_size
        self.cache.release(slot)
        self.cache.adopt(slot, pages)
        self.seen[slot] = 0
        if tokens:
            self.seen[slot, torch.tensor(tokens, device=self.device, dtype=torch.long)] = 1

    pipelined = True  # supports decode_async (the TP CollectiveRunner does not)

    @torch.no_grad()
    def decode(self, rows: list[dict]):
        """rows: [{token, pos, slot, temperature, top_k, top_p, rep, seed, bans}]
        -> (ids list[int], logprobs list[float]) of the next token per row."""
        return self.decode_async(rows).result()

    @torch.no_grad()
    def decode_async(self, rows: list[dict], prev: DecodeHandle | None = None) -> DecodeHandle:
        """Launch one decode step without waiting for it. A row whose
        ``token`` is None takes its input token from ``prev``'s output row
        ``src`` on the device (the previous step's sample, not yet seen by the
        host), so the engine can launch step t+1 before reading step t: the GPU
        never idles on the host's bookkeeping between steps."""
        n = len(rows)
        Bb = _next_pow2(n)
        max_kv = max(r["pos"] for r in rows) + 1
        Kb = min(_next_pow2(max_kv, 256), self.max_len)
        if self.device.type != "cuda":
            Bb = n  # GPU eager keeps the graph buckets so both paths run identical shapes
        st = self._static_for(Bb, Kb)
        pk = st["pk"]
        pk.flip()
        NB = self.max_bans
        for r in rows:
            self.cache.reserve(r["slot"], r["pos"] + 1)
        self.cache.sync()
        a = pk.np
        tok, sd, pos, sl, kl = a["tokens"], a["seeds"], a["pos"], a["slots"], a["kv_lens"]
        tk, te, tp, rp, bans = a["top_k"], a["temperature"], a["top_p"], a["rep"], a["bans"]
        bans.fill(-1)
        ch = a["chain"]
        ch.fill(-1)
        chain_dst, chain_src = [], []
        for i in range(Bb):
            if i < n:
                r = rows[i]
                t = r["token"]
                if t is None:
                    chain_dst.append(i)
                    chain_src.append(int(r["src"]))
                    t = 0
                tok[i], pos[i], sl[i], kl[i] = t, r["pos"], r["slot"], r["pos"] + 1
                te[i], tk[i], tp[i], rp[i] = r["temperature"], r["top_k"], r["top_p"], r["rep"]
                sd[i] = r["seed"]
                b = r.get("bans") or ()
                if len(b) > NB:
                    raise ValueError(f"{len(b)} banned ids > max_bans={NB}")
                for j, t in enumerate(b):
                    bans[i * NB + j] = t
            else:  # padding row -> scratch slot
                tok[i], pos[i], sl[i], kl[i] = 0, 0, self.cache.scratch, 1
                te[i], tk[i], tp[i], rp[i], sd[i] = 0.0, 0, 1.0, 1.0, 0
        if "rcos" in pk.fields or "pages" in pk.fields:
            self._fill_desc(a, Bb, pos, sl)
        # every row (padding rows are greedy) on the multi-workgroup sampler: no closing kernel; the
        # step graphs are keyed by it too
        mc = bool(((~(te[:Bb] > 0)) | ((tk[:Bb] >= 1) & (tk[:Bb] <= dops.MWG_KMAX))).all())
        gk = (Bb, Kb, mc)
        if chain_dst and prev is None:
            raise ValueError("rows chain their token from a previous launch, but prev is None")
        # chained tokens read on the device by the step's first kernel: the previous step wrote them into
        # this bucket's shared output buffer (same batch bucket); otherwise copied into `tokens` below
        # (not on a step that captures its graph: the capture's eager warm-up runs would read the chained
        # token from the output buffer their own first run already overwrote)
        fold = (bool(chain_dst) and Bb == 1 and self._embed_head
                and prev.ids_dev.data_ptr() == st["ids"].data_ptr()
                and (not self.use_graphs or gk in self._graphs))
        if fold:
            for d_, s_ in zip(chain_dst, chain_src):
                ch[d_] = s_
        pk.upload()
        if chain_dst and not fold:
            dst = pk.d("tokens")
            m = len(chain_dst)
            if chain_dst == chain_src == list(range(m)):  # the common case: same rows, same order
                dst[:m].copy_(prev.ids_dev[:m])
            else:
                di = torch.tensor(chain_dst, dtype=torch.long).to(self.device, non_blocking=True)
                si = torch.tensor(chain_src, dtype=torch.long).to(self.device, non_blocking=True)
                dst.index_copy_(0, di, prev.ids_dev.index_select(0, si))
        if self.use_graphs:
            g = self._graphs.get(gk)
            if g is None:
                g = self._capture(st, Bb, Kb, mc)
            g.replay()
        else:
            self._step_body(st, Bb, Kb, mc)
        fl = st["flip"]
        fl[0] ^= 1
        k = fl[0]
        ids_h, lps_h = st["ids_h"][k], st["lps_h"][k]
        if self.device.type == "cuda":
            st["out_h"][k].copy_(st["out"], non_blocking=True)  # ids + log-probs, one copy
            ev = torch.cuda.Event()
            ev.record()
        else:
            st["out_h"][k].copy_(st["out"])
            ev = None
        return DecodeHandle(ids_h, lps_h, n, ev, st["ids"])

    def _capture(self, st, Bb, Kb, mc=False, body=None, key=None):
        """Capture a step into a graph: the decode step, or ``body`` (the verify step) under ``key``."""
        body = body or self._step_body
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warm up (allocator, hipBLASLt heuristics)
                body(st, Bb, Kb, mc)
        torch.cuda.current_stream().wait_stream(s)
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        # thread-local capture: the RCCL process-group watchdog thread polls its work events while a
        # capture runs; under the default global mode that query fails ("operation not permitted when
        # stream is capturing") and the watchdog aborts the process
        with torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
            body(st, Bb, Kb, mc)
        self._graphs[key or (Bb, Kb, mc)] = g
        return g

    # -------------------------------------------------------------- verify
    def _spec_static_for(self, Bb: int, Kb: int):
        """Static buffers of a verify bucket: Bb sequences x T rows, kv bucket Kb (apart from decode's)."""
        T = self.spec_tokens
        key = ("spec", Bb, T, Kb)
        st = self._static.get(key)
        if st is not None:
            return st
        M, NB = Bb * T, self.max_bans
        pk = _Packed({"tokens": (torch.int64, M), "seeds": (torch.int64, M), "pos": (torch.int32, M),
                      "base": (torch.int32, Bb), "n_tok": (torch.int32, Bb), "slots": (torch.int32, Bb),
                      "kv_lens": (torch.int32, Bb), "row_slots": (torch.int32, M), "row_kv": (torch.int32, M),
                      "seen_slots": (torch.int32, M), "top_k": (torch.int32, M), "temperature": (torch.float32, M),
                      "top_p": (torch.float32, M), "rep": (torch.float32, M), "bans": (torch.int32, M * NB)},
                     self.device)
        ws_n = max(spec.spec_ws_floats(Bb, T, self.H, self.Hkv, self.D, Kb),
                   dops.decode_ws_floats(M, self.H, self.Hkv, self.D, Kb))  # (either arm: _spec_rows)
        st = {"pk": pk, "ws": torch.zeros(max(ws_n, 1), device=self.device, dtype=torch.float32),
              "obuf": torch.empty(M, self.H * self.D, device=self.device, dtype=self.dtype),
              "sws": torch.empty(M * self.V, device=self.device, dtype=torch.float32),
              **self._outbuf(M, key=("spec", M))}
        self._static[key] = st
        return st

    def _spec_rows(self, Bb: int, Kb: int) -> bool:
        """Whether a verify bucket runs its attention as Bb * T rows of ``kca_decode_attn`` -- row (b, t) a
        sequence of length pos + t + 1 -- after ``kca_spec_prep``, instead of ``kca_spec_attn``. The
        multi-token kernel reads each K/V row once for T queries but has 1/T of the workgroups and T times
        the arithmetic per workgroup; on a short KV stream that chain is longer than streaming the rows T
        times (docs/PERF.md, Round 12: it loses at T >= 4 up to 65536 (sequence, kv-head, position) rows
        and wins from 114688 on). bf16 only: ``kca_decode_attn`` has no fp16 twin."""
        return (self.spec_tokens >= 4 and self.dtype == torch.bfloat16 and self.device.type == "cuda"
                and Bb * self.Hkv * Kb <= self._spec_rows_work)

    def _spec_step_body(self, st, Bb, Kb, mc=False):
        """One verify step: the layer code on Bb * T rows with the attention switched to the multi-token
        kernels (_attn), then the sampler on every row. The sampler's repetition mask: a row that may be
        rejected must not mark it, so every row points at the scratch slot's mask row except the single
        row of a request with a repetition penalty (such a request is never given drafts)."""
        pk, T = st["pk"], self.spec_tokens
        n0 = _lib.LAUNCHES[0]
        self.spec_steps += 1
        self._chain_src, self._step_desc = None, None
        rows = (pk.d("row_slots"), pk.d("row_kv")) if self._spec_rows(Bb, Kb) else None
        self.spec_rows_steps += rows is not None
        self._spec = (pk.d("base"), pk.d("n_tok"), pk.d("slots"), pk.d("kv_lens"), T, rows)
        try:
            logits = self._layers_decode(pk.d("tokens"), pk.d("pos"), pk.d("slots"), pk.d("kv_lens"), Kb,
                                         st["ws"], st["obuf"])
        finally:
            self._spec = None
        dops.sample_logits(logits, temperature=pk.d("temperature"), top_k=pk.d("top_k"), top_p=pk.d("top_p"),
                           rep_penalty=pk.d("rep"), seen=self.seen, slots=pk.d("seen_slots"),
                           ban_ids=pk.d("bans").view(Bb * T, self.max_bans), seeds=pk.d("seeds"), step=0,
                           ws=st["sws"], out_ids=st["ids"], out_logprobs=st["lps"], mwg_complete=mc)
        self.step_launches[("spec", Bb, T)] = _lib.LAUNCHES[0] - n0

    @torch.no_grad()
    def verify(self, rows: list[dict]):
        """rows: [{tokens: [t0, d1, .., d_{n-1}], pos, slot, temperature, top_k, top_p, rep, seeds: [n],
        bans: [n lists]}], 1 <= n <= ``spec_tokens``: ``t0`` is the sequence's last token (position ``pos``,
        its K/V not yet cached, as in ``decode``), ``d_i`` the drafted tokens after it. -> (ids, logprobs):
        per row the n tokens sampled after ``t0``, after ``t0 d1``, ... and their log-probs. Sample t is
        valid only if the drafts before it were right (d_i == sample i-1): the caller stops at the first
        mismatch; the rejected rows' K/V stay past the sequence's length until overwritten."""
        return self.verify_async(rows).result()

    @torch.no_grad()
    def verify_async(self, rows: list[dict]) -> "VerifyHandle":
        """Launch one verify step without waiting for it (inputs in one packed H2D copy, outputs in one
        D2H copy behind an event, as ``decode_async``)."""
        T = self.spec_tokens
        if not T:
            raise RuntimeError("verify needs spec_tokens (KCA_DECODE_SPEC) set on the runner")
        n = len(rows)
        ns = [len(r["tokens"]) for r in rows]
        if not all(1 <= k <= T for k in ns):
            raise ValueError(f"a verify row takes 1..{T} tokens, got {ns}")
        if any(r["pos"] + k > self.max_len for r, k in zip(rows, ns)):
            raise ValueError("a verify row would write past max_len")
        Bb = _next_pow2(n) if self.device.type == "cuda" else n
        max_kv = max(r["pos"] + k for r, k in zip(rows, ns))
        Kb = min(_next_pow2(max_kv, 256), self.max_len)
        st = self._spec_static_for(Bb, Kb)
        pk = st["pk"]
        pk.flip()
        NB, M = self.max_bans, Bb * T
        for r, k in zip(rows, ns):
            self.cache.reserve(r["slot"], r["pos"] + k)
        self.cache.sync()
        a = pk.np
        a["bans"].fill(-1)
        a["tokens"].fill(0)
        a["seeds"].fill(0)
        a["temperature"].fill(0.0)
        a["top_k"].fill(0)
        a["top_p"].fill(1.0)
        a["rep"].fill(1.0)
        scratch = self.cache.scratch
        a["seen_slots"].fill(scratch)
        a["pos"].fill(0)  # (a padding row: token 0 at position 0 to every kernel but the attention, which skips it
        a["row_slots"].fill(scratch)  # -- or, on the rows arm, reads one row of the scratch slot)
        a["row_kv"].fill(1)
        for i in range(Bb):
            if i >= n:  # padding sequence -> scratch slot
                a["base"][i], a["n_tok"][i], a["slots"][i], a["kv_lens"][i] = 0, 1, scratch, 1
                continue
            r, k = rows[i], ns[i]
            a["base"][i], a["n_tok"][i], a["slots"][i], a["kv_lens"][i] = r["pos"], k, r["slot"], r["pos"] + k
            rp = float(r.get("rep", 1.0) or 1.0)
            if rp != 1.0 and k != 1:
                raise ValueError("a request with a repetition penalty verifies one token at a time")
            if len(r["seeds"]) != k or len(r.get("bans") or [()] * k) != k:
                raise ValueError("a verify row needs one seed and one ban list per token")
            for t in range(k):
                j = i * T + t
                a["tokens"][j], a["pos"][j], a["seeds"][j] = r["tokens"][t], r["pos"] + t, r["seeds"][t]
                a["row_slots"][j], a["row_kv"][j] = r["slot"], r["pos"] + t + 1
                a["temperature"][j], a["top_k"][j], a["top_p"][j] = r["temperature"], r["top_k"], r["top_p"]
                b = (r.get("bans") or [()] * k)[t] or ()
                if len(b) > NB:
                    raise ValueError(f"{len(b)} banned ids > max_bans={NB}")
                for jj, tok in enumerate(b):
                    a["bans"][j * NB + jj] = tok
            if rp != 1.0:
                a["rep"][i * T], a["seen_slots"][i * T] = rp, r["slot"]
        te, tk = a["temperature"], a["top_k"]
        mc = bool(((~(te[:M] > 0)) | ((tk[:M] >= 1) & (tk[:M] <= dops.MWG_KMAX))).all())
        pk.upload()
        if self.use_graphs:
            gk = ("spec", Bb, T, Kb, mc)
            g = self._graphs.get(gk)
            if g is None:
                g = self._capture(st, Bb, Kb, mc, body=self._spec_step_body, key=gk)
            g.replay()
        else:
            self._spec_step_body(st, Bb, Kb, mc)
        fl = st["flip"]
        fl[0] ^= 1
        k = fl[0]
        if self.device.type == "cuda":
            st["out_h"][k].copy_(st["out"], non_blocking=True)  # ids + log-probs, one copy
            ev = torch.cuda.Event()
            ev.record()
        else:
            st["out_h"][k].copy_(st["out"])
            ev = None
        return VerifyHandle(DecodeHandle(st["ids_h"][k], st["lps_h"][k], M, ev, st["ids"]), ns, T)

    @torch.no_grad()
    def sample_first(self, logits: torch.Tensor, rows: list[dict]):
        """Sample from prefill logits [n, V] (row params as in ``decode``)."""
        n = logits.shape[0]
        dev = self.device
        NB = self.max_bans
        bans = torch.full((n, NB), -1, dtype=torch.int32)
        for i, r in enumerate(rows):
            for j, t in enumerate((r.get("bans") or ())[:NB]):
                bans[i, j] = t
        f = lambda k, dt: torch.tensor([r[k] for r in rows], dtype=dt, device=dev)  # noqa: E731
        ids, lps = dops.sample_logits(
            logits.contiguous(), temperature=f("temperature", torch.float32), top_k=f("top_k", torch.int32),
            top_p=f("top_p", torch.float32), rep_penalty=f("rep", torch.float32), seen=self.seen,
            slots=f("slot", torch.int32), ban_ids=bans.to(dev), seeds=f("seed", torch.int64), step=0,
            mwg_complete=dops.mwg_complete_rows([r["temperature"] for r in rows], [r["top_k"] for r in rows]))
        return ids.tolist(), lps.tolist()


def mix_seed(seed: int, step: int) -> int:
    """Per-(request, token) 64-bit Philox key as a signed int64."""
    x = (seed * 0x9E3779B97F4A7C15 + (step + 1) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x ^= x >> 31
    x = (x * 0x94D049BB133111EB) & ((1 << 64) - 1)
    x ^= x >> 29
    return x - (1 << 64) if x >= (1 << 63) else x


__all__ = ["KVCache", "KVCacheFull", "ModelRunner", "DecodeHandle", "VerifyHandle", "mix_seed", "math"]
