// Prefill attention over the KV cache (prefix caching, chunked prefill): the queries of a prompt chunk
// attend to keys that are read through the block table.
//
//   kca_prefill_paged_attn   row r of the launch holds lens[r] queries (of T padded ones); query i sits at
//                            position start[r] + i and attends keys [0, start[r] + i] of slot slots[r].
//                            EVERY key comes from the cache -- the chunk's own K/V were written just before
//                            (KVCache.write) and are exact in the 16-bit cache. ALiBi slope * (key - qpos),
//                            GQA by H / Hkv. Queries i >= lens[r] come out as zeros.
//
// The design is attention.hip's forward (its header has the reasoning): swapped v_mfma_f32_32x32x16
// products with the query on the lane, a lane-local online softmax with the deferred rescale, 4 waves x
// 32 queries per workgroup, 32-key K/V tiles register-staged into the padded LDS images (next tile's loads
// in flight under this tile's MFMAs), V^T by ds_read_b64_tr_b16. What differs:
//
//   * the tile loader is a table lookup. Pages hold PS = 2^shift >= 16 positions and tiles start at
//     multiples of 32, so each half tile (16 keys) lies in one page: two workgroup-uniform page ids per
//     tile, and every (page, head) is one contiguous run of rows. The contiguous cache is the same loader
//     with the slot as the only "page".
//   * rows at or past the tile's causal limit are never loaded (they may be unwritten, NaN, or belong to a
//     page the slot does not own): their LDS rows are zeros, so a weight of 0 meets a V of 0.
//   * DT = 1 instantiates the f16 MFMA (skinny_mfma.hip, decode_spec.hip); P <= 2^8 between rescales fits
//     fp16 as it fits bf16. fp16 outputs are held to two units in the last place of the OUTPUT, which a
//     P rounded once to fp16 (2^-11 of sum p |v|) misses wherever the sum cancels, so the fp16 kernel
//     feeds P as two fp16 terms, fp16(P) and fp16(P - fp16(P)): two P.V products per V fragment, fp32
//     accumulation, P good to 2^-22. bf16 keeps one term (its bound is relative to sum p |v|).
//   * grid (query tile, head, row); a workgroup whose tile starts at or past lens[r] writes zeros and
//     exits; the key loop ends at the tile's own causal limit start + min(lens, tile end). No LSE.
//   * the G query heads of a KV head are separate workgroups: they run side by side (heads are the second
//     grid dimension) and share the K/V stream through L2, which keeps the softmax state at one head per
//     wave -- 4 x G queries per lane would not fit the registers of D = 256.
//
// No atomics and no workspace: a workgroup reads only its row's slot and writes only its own outputs, so
// the result is deterministic and independent of the other rows of the launch.
// Head dims are padded to a compiled D in {64, 96, 128, 160, 256} as in attention.hip.
#include <algorithm>

#include "common.h"

#define PP_LOG2E 1.4426950408889634f
#define PP_RESCALE_THR 8.0f

typedef _Float16 pp_f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) bf16x4 pp_lds_bf16x4;

struct PrefillPagedParams {
  const uint16_t* q;
  uint16_t* o;
  const uint16_t* kc;
  const uint16_t* vc;
  long long q_sb, q_st, q_sh, o_sb, o_st, o_sh;
  long long cs_slot, cs_head, cs_pos;
  const int* slots;
  const int* start;
  const int* lens;
  const int* tbl;
  const float* alibi;
  int tbl_stride, ps_shift;
  int n_slots, n_blocks, max_pos;
  int T, H, Hkv, d_real;
  float scale;
};

template <int DT>
__device__ __forceinline__ f32x16 pp_mfma(uint4 a, uint4 b, f32x16 c) {
  if constexpr (DT == 0)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(pp_f16x8, a), __builtin_bit_cast(pp_f16x8, b), c,
                                                  0, 0, 0);
}

template <int DT>
__device__ __forceinline__ uint32_t pp_pack2(float lo, float hi) {
  return f2e<DT>(lo) | (f2e<DT>(hi) << 16);
}

template <int DT>
__device__ __forceinline__ uint4 pp_pack8(const float* x) {
  return make_uint4(pp_pack2<DT>(x[0], x[1]), pp_pack2<DT>(x[2], x[3]), pp_pack2<DT>(x[4], x[5]),
                    pp_pack2<DT>(x[6], x[7]));
}

// the transposed 4 x 16-bit read: element-type agnostic (it moves bits)
__device__ __forceinline__ uint2 pp_tr_read(const uint16_t* lds_ptr) {
  return __builtin_bit_cast(
      uint2, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((pp_lds_bf16x4*)(reinterpret_cast<uintptr_t>(lds_ptr))));
}

// attention.hip FwdLds: bank-conflict-free row strides (in elements)
template <int D> struct PPLds {
  static constexpr int KSTR = D + 8;
  static constexpr int VPADB = ((64 - (2 * D) % 256 + 256) % 256) < ((192 - (2 * D) % 256 + 256) % 256)
                                   ? ((64 - (2 * D) % 256 + 256) % 256)
                                   : ((192 - (2 * D) % 256 + 256) % 256);
  static constexpr int VSTR = D + VPADB / 2;
};

// The 32 keys [k0, k0 + 32) of one kv head, 16 B chunks in registers. offA / offB: element offsets of
// the rows of keys k0 and k0 + 16 (each half tile is one contiguous run); a row at or past `limit`, a
// chunk at or past d_real and a half tile whose offset is negative (no such page) are zeros.
template <int D>
struct PPStager {
  static constexpr int NC = D / 8;
  static constexpr int TOTAL = 32 * NC;
  static constexpr int CPT = (TOTAL + 255) / 256;
  uint4 r[CPT];
  __device__ __forceinline__ void load(const uint16_t* base, long long offA, long long offB, long long cs_pos, int k0,
                                       int limit, int d_real) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int idx = threadIdx.x + i * 256;
      const int row = idx / NC, ch = idx % NC;
      const long long off = row < 16 ? offA : offB;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (idx < TOTAL && k0 + row < limit && ch * 8 < d_real && off >= 0)
        val = *reinterpret_cast<const uint4*>(base + off + (long long)(row & 15) * cs_pos + ch * 8);
      r[i] = val;
    }
  }
  __device__ __forceinline__ void store(uint16_t* lds, int stride) const {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int idx = threadIdx.x + i * 256;
      if (TOTAL % 256 == 0 || idx < TOTAL) {
        const int row = idx / NC, ch = idx % NC;
        *reinterpret_cast<uint4*>(lds + row * stride + ch * 8) = r[i];
      }
    }
  }
};

template <int D, int DT>
__global__ void __launch_bounds__(256, (D <= 128 ? 2 : 1)) prefill_paged_kernel(PrefillPagedParams p) {
  using L = PPLds<D>;
  constexpr int BM = 128, BN = 32;
  constexpr int KSZ = BN * L::KSTR, VSZ = BN * L::VSTR;
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * (KSZ + VSZ)];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int qb = (int)gridDim.x - 1 - (int)blockIdx.x;  // the longest key loops first
  const int h = blockIdx.y, r = blockIdx.z;
  const int hk = h / (p.H / p.Hkv);
  const int slot = p.slots[r];
  const bool slot_ok = slot >= 0 && slot < p.n_slots;
  KCA_DASSERT(slot_ok);
  const int st = max(p.start[r], 0);
  // queries of the row, cut to what the slot can hold (positions < max_pos)
  const int len = slot_ok ? max(0, min(min(p.lens[r], p.T), p.max_pos - st)) : 0;
  uint16_t* ob = p.o + r * p.o_sb + h * p.o_sh;

  if (qb * BM >= len) {  // workgroup-uniform: a tile of padding queries
    const int nc = p.d_real / 8;
    const int rows = min(BM, p.T - qb * BM);
    for (int idx = threadIdx.x; idx < rows * nc; idx += 256) {
      const int row = qb * BM + idx / nc, ch = idx % nc;
      *reinterpret_cast<uint4*>(ob + (long long)row * p.o_st + ch * 8) = make_uint4(0, 0, 0, 0);
    }
    return;
  }

  const int q0 = qb * BM + wave * BN;
  const int qrow = q0 + l32;
  const int kv_hi = st + min(len, qb * BM + BM);  // one past the last key the tile's last query sees
  const int ntiles = (kv_hi + BN - 1) / BN;
  const float sl2 = p.scale * PP_LOG2E;
  const float slope = p.alibi ? p.alibi[h] * PP_LOG2E : 0.f;
  const uint16_t* kp = p.kc + hk * p.cs_head;
  const uint16_t* vp = p.vc + hk * p.cs_head;
  const int pmask = (1 << p.ps_shift) - 1;

  // element offset of key kk's row (kk a multiple of 16, workgroup-uniform); -1: nothing to read
  auto run_off = [&](int kk) -> long long {
    if (kk >= kv_hi) return -1;
    if (p.tbl) {
      const int page = p.tbl[(long long)slot * p.tbl_stride + (kk >> p.ps_shift)];
      KCA_DASSERT(page >= 0 && page < p.n_blocks);
      if (page < 0 || page >= p.n_blocks) return -1;
      return (long long)page * p.cs_slot + (long long)(kk & pmask) * p.cs_pos;
    }
    return (long long)slot * p.cs_slot + (long long)kk * p.cs_pos;
  };

  const uint16_t* qp = p.q + r * p.q_sb + h * p.q_sh + (long long)qrow * p.q_st;
  uint4 qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const int d0 = 16 * s + 8 * hh;
    qf[s] = (qrow < len && d0 < p.d_real) ? *reinterpret_cast<const uint4*>(qp + d0) : make_uint4(0, 0, 0, 0);
  }
  f32x16 oacc[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) oacc[i][j] = 0.f;
  float m = -INFINITY, lsum = 0.f;

  PPStager<D> sk, sv;
  {
    const long long oa = run_off(0), ob_ = run_off(16);
    sk.load(kp, oa, ob_, p.cs_pos, 0, kv_hi, p.d_real);
    sv.load(vp, oa, ob_, p.cs_pos, 0, kv_hi, p.d_real);
    sk.store(smem, L::KSTR);
    sv.store(smem + KSZ, L::VSTR);
  }
  __syncthreads();

  const int gi = lane & 15;
  const int dcol = 16 * ((lane >> 4) & 1) + 4 * (gi & 3);
  const int qpos = st + qrow;
  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * BN;
    const uint16_t* Ks = smem + (t & 1) * (KSZ + VSZ);
    const uint16_t* Vs = Ks + KSZ;
    if (t + 1 < ntiles) {  // next tile's loads in flight under this tile's MFMAs
      const long long oa = run_off(k0 + BN), ob_ = run_off(k0 + BN + 16);
      sk.load(kp, oa, ob_, p.cs_pos, k0 + BN, kv_hi, p.d_real);
      sv.load(vp, oa, ob_, p.cs_pos, k0 + BN, kv_hi, p.d_real);
    }
    const bool active = q0 < len && k0 <= st + q0 + BN - 1;
    if (active) {
      f32x16 sacc;
#pragma unroll
      for (int j = 0; j < 16; ++j) sacc[j] = 0.f;
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        const uint4 a = *reinterpret_cast<const uint4*>(Ks + l32 * L::KSTR + 16 * s + 8 * hh);
        sacc = pp_mfma<DT>(a, qf[s], sacc);
      }
      const bool need_mask = (k0 + BN - 1 > st + q0) || (k0 + BN > kv_hi);
      float x[16];
      float mt = -INFINITY;
      if (need_mask || p.alibi) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int key = k0 + (j & 3) + 8 * (j >> 2) + 4 * hh;
          const bool valid = key <= qpos && key < kv_hi && qrow < len;
          float v = sacc[j] * sl2;
          if (p.alibi) v += slope * (float)(key - qpos);
          x[j] = valid ? v : -INFINITY;
          mt = fmaxf(mt, x[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          x[j] = sacc[j] * sl2;
          mt = fmaxf(mt, x[j]);
        }
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      if (!__all(mt <= m + PP_RESCALE_THR)) {
        const float mnew = fmaxf(m, mt);
        const float alpha = (mnew == -INFINITY) ? 1.f : exp2f(m - mnew);
        lsum *= alpha;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
          for (int j = 0; j < 16; ++j) oacc[i][j] *= alpha;
        m = mnew;
      }
      const float msub = (m == -INFINITY) ? 0.f : m;
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        x[j] = exp2f(x[j] - msub);
        ps += x[j];
      }
      lsum += ps;
      const uint4 pf0 = pp_pack8<DT>(x), pf1 = pp_pack8<DT>(x + 8);
      uint4 pr0, pr1;  // fp16 only: P - fp16(P), the second half of a two-term P (header comment)
      if constexpr (DT == 1) {
        float xr[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xr[j] = x[j] - (float)(_Float16)x[j];
        pr0 = pp_pack8<DT>(xr);
        pr1 = pp_pack8<DT>(xr + 8);
      }
#pragma unroll
      for (int db = 0; db < D / 32; ++db) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int row = 16 * s + 4 * hh + (gi >> 2);
          const uint16_t* vb = Vs + row * L::VSTR + db * 32 + dcol;
          const uint2 lo = pp_tr_read(vb), hi = pp_tr_read(vb + 8 * L::VSTR);
          const uint4 vt = make_uint4(lo.x, lo.y, hi.x, hi.y);
          oacc[db] = pp_mfma<DT>(vt, s ? pf1 : pf0, oacc[db]);
          if constexpr (DT == 1) oacc[db] = pp_mfma<DT>(vt, s ? pr1 : pr0, oacc[db]);
        }
      }
    }
    if (t + 1 < ntiles) {  // the other buffer: last read in tile t - 1, fenced by its barrier
      uint16_t* Kn = smem + ((t + 1) & 1) * (KSZ + VSZ);
      sk.store(Kn, L::KSTR);
      sv.store(Kn + KSZ, L::VSTR);
    }
    __syncthreads();
  }

  const float ltot = lsum + __shfl_xor(lsum, 32, 64);
  const float inv = (qrow < len && ltot > 0.f) ? 1.f / ltot : 0.f;
  if (qrow < p.T) {  // padding queries of a live tile: zeros (their accumulators never left 0)
    uint16_t* op = ob + (long long)qrow * p.o_st;
#pragma unroll
    for (int db = 0; db < D / 32; ++db) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hh;
        if (d < p.d_real) {
          uint2 w;
          w.x = pp_pack2<DT>(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
          w.y = pp_pack2<DT>(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
          *reinterpret_cast<uint2*>(op + d) = w;
        }
      }
    }
  }
}

template <int D, int DT>
static void pp_launch(const PrefillPagedParams& p, int n, hipStream_t stream) {
  const dim3 grid((unsigned)((p.T + 127) / 128), (unsigned)p.H, (unsigned)n);
  hipLaunchKernelGGL((prefill_paged_kernel<D, DT>), grid, dim3(256), 0, stream, p);
}

template <int DT>
static int pp_launch_d(const PrefillPagedParams& p, int n, hipStream_t stream) {
  const int d = p.d_real;
  if (d <= 64) pp_launch<64, DT>(p, n, stream);
  else if (d <= 96) pp_launch<96, DT>(p, n, stream);
  else if (d <= 128) pp_launch<128, DT>(p, n, stream);
  else if (d <= 160) pp_launch<160, DT>(p, n, stream);
  else pp_launch<256, DT>(p, n, stream);
  return 0;
}

// q / out: [n, T, H, D] views (row, token and head strides in elements). kc / vc: the layer's caches,
// [n_blocks, Hkv, PS or max_len, D] with strides cs_slot / cs_head / cs_pos; tbl [n_slots, tbl_stride] page
// ids (null: contiguous, the slot is the block and n_slots == n_blocks). max_pos: positions a slot holds.
KCA_API int kca_prefill_paged_attn(const void* q, long long q_sb, long long q_st, long long q_sh, void* out,
                                   long long o_sb, long long o_st, long long o_sh, const void* kc, const void* vc,
                                   long long cs_slot, long long cs_head, long long cs_pos, const int* slots,
                                   const int* start, const int* lens, int n, int T, int H, int Hkv, int D, float scale,
                                   const float* alibi, const int* tbl, int tbl_stride, int ps_shift, int n_slots,
                                   int n_blocks, int max_pos, int dt, hipStream_t stream) {
  if (D <= 0 || D % 8 || D > 256 || H <= 0 || Hkv <= 0 || H % Hkv || n <= 0 || T <= 0) return 1;
  if (dt != 0 && dt != 1) return 2;
  if (H > 65535 || n > 65535) return 3;  // grid y / z
  if (tbl && (ps_shift < 4 || ps_shift > 20 || tbl_stride <= 0)) return 5;  // pages of >= 16 positions
  if (n_slots <= 0 || n_blocks <= 0 || max_pos <= 0) return 1;
  // a lane's eight elements are one aligned 16-byte access
  if ((q_sb | q_st | q_sh | o_sb | o_st | o_sh | cs_slot | cs_head | cs_pos) % 8) return 1;
  if (((uintptr_t)q | (uintptr_t)out | (uintptr_t)kc | (uintptr_t)vc) % 16) return 1;
  if (tbl) max_pos = (int)std::min((long long)max_pos, (long long)tbl_stride << ps_shift);
  else if (cs_pos > 0) max_pos = (int)std::min((long long)max_pos, cs_head / cs_pos);
  if (!tbl) ps_shift = 30;
  PrefillPagedParams p{(const uint16_t*)q, (uint16_t*)out, (const uint16_t*)kc, (const uint16_t*)vc, q_sb, q_st, q_sh,
                       o_sb, o_st, o_sh, cs_slot, cs_head, cs_pos, slots, start, lens, tbl, alibi, tbl_stride,
                       ps_shift, n_slots, n_blocks, max_pos, T, H, Hkv, D, scale};
  return dt == 1 ? pp_launch_d<1>(p, n, stream) : pp_launch_d<0>(p, n, stream);
}
