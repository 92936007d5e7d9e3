// FP8 KV cache for decode: e4m3 K/V rows with one fp32 scale per (token, kv-head) row.
//
//   kca_kv8_prep   RoPE on the step's Q (in place) and K, then K and V rows quantized -- scale =
//                  absmax / 448 (1 for an all-zero row), the fp32 quotient clamped to +-448 and packed
//                  by v_cvt_pk_fp8_f32 (OCP e4m3fn on gfx950, round to nearest even) -- and appended to
//                  the byte cache with their scales (ops/kv8.py quantize_rows is the contract)
//   kca_kv8_attn   split-K decode attention of one query token per sequence over the byte cache:
//                  score(t) = scale * k_scale[t] * sum_d q[d] k8[t, d] + ALiBi,
//                  out = sum_t p[t] v_scale[t] v8[t, :] / sum_t p[t], fp32 throughout, one rounding;
//                  the row scales multiply fp32 sums, never the bytes (ops/kv8.py
//                  kv8_attention_reference). Splits leave (O, max, sum) partials in the fp32 workspace
//                  and kv8_combine_kernel folds them in split order, so the same inputs give the same
//                  bits and launches on separate workspaces share nothing.
//
// Cache layout: the 16-bit cache's (decode.hip), one byte per element: [slot][kv_head][pos][D] uint8
// (strides passed in) plus scales [slot][kv_head][pos] fp32 (unit position stride); paged pools
// [page][kv_head][ps][D] / [page][kv_head][ps] addressed through the same block table.
//
// Lane layout of the attention kernel: 8 bytes (8 dims) of a row per lane, LPT = 8 / 16 / 32 lanes per
// token row -- the 16-bit kernel's dims-per-lane, so q and the P.V accumulator cost the same registers
// per GQA head (G = 8 stays clear of scratch; 16 bytes per lane would double both) and a wave step
// still covers 64 / LPT rows: with U = 4 a lane keeps 2U 8-byte row loads in flight, the same number
// of rows as the 16-bit kernel's 2U 16-byte loads, at half the bytes per row. A token's two scales are
// one 4-byte load each per lane (the lanes of a row read the same word), not one per dim.
//
// Launches per layer: prep, attention, and the combine when the cache spans more than one split.
#include <algorithm>

#include "common.h"

extern "C" int kca_decode_chunk(int B, int Hkv, int max_kv);  // decode.hip: the split size

// byte offset of token t's rows inside a head, and the offset of its scale (paged or contiguous)
__device__ __forceinline__ void kv8_row(const int* __restrict__ tbl, int tbl_stride, int ps_shift, int seq, int t,
                                        long long cs_slot, long long cs_pos, long long ss_slot, long long& boff,
                                        long long& soff) {
  long long base = seq;
  int tt = t;
  if (tbl) {
    base = tbl[(long long)seq * tbl_stride + (t >> ps_shift)];
    tt = t & ((1 << ps_shift) - 1);
  }
  KCA_DASSERT(base >= 0);
  boff = base * cs_slot + (long long)tt * cs_pos;
  soff = base * ss_slot + tt;
}

// ------------------------------------------------------------------ prep
// One wave per (b, head-row) of the fused QKV output [B, (H+2Hkv)*D]; a lane owns the 4 consecutive
// dims [4 lane, 4 lane + 4) (D <= 256), so its four e4m3 bytes are one 32-bit store. Rotation partners
// are read from the unrotated row, and every lane loads before any lane stores (one wave per row).
template <int DT>
__global__ __launch_bounds__(256) void kv8_prep_kernel(
    uint16_t* __restrict__ qkv, long long ld, int B, int H, int Hkv, int D, int rot, int interleaved,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, const int* __restrict__ pos,
    const int* __restrict__ slots, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ks,
    float* __restrict__ vs, long long cs_slot, long long cs_head, long long cs_pos, long long ss_slot,
    long long ss_head, const int* __restrict__ tbl, int tbl_stride, int ps_shift) {
  const int rows_per_b = H + 2 * Hkv;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)B * rows_per_b) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / rows_per_b), j = (int)(row % rows_per_b);
  uint16_t* src = qkv + b * ld + (long long)j * D;
  const int p = pos[b];
  KCA_DASSERT(p >= 0 && (tbl || (long long)p * cs_pos < cs_head));
  const int d0 = lane * 4;
  const bool act = d0 < D;  // D % 4 == 0: a lane is inside the row or outside it
  float x[4], y[4];
  const int half = rot >> 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = d0 + i;
    x[i] = 0.f;
    y[i] = 0.f;
    if (act) {
      x[i] = e2f<DT>(src[d]);
      y[i] = x[i];
      if (j < H + Hkv && d < rot) {
        int partner, fi;
        float sgn;
        if (interleaved) {
          partner = d ^ 1;
          fi = d >> 1;
          sgn = (d & 1) ? 1.f : -1.f;
        } else {
          partner = d < half ? d + half : d - half;
          fi = d < half ? d : d - half;
          sgn = d < half ? -1.f : 1.f;
        }
        const float xp = e2f<DT>(src[partner]);
        const float c = cos_t[(long long)p * half + fi], s = sin_t[(long long)p * half + fi];
        y[i] = x[i] * c + sgn * xp * s;
      }
    }
  }
  if (j < H) {  // query: rotate in place (only if rotary)
    if (rot > 0 && act) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (d0 + i < rot) src[d0 + i] = (uint16_t)f2e<DT>(y[i]);
    }
    return;
  }
  const bool is_k = j < H + Hkv;
  // the row the 16-bit cache would hold (the rotated K rounded to the element type; V as it is), a
  // non-finite value counted as 0
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = is_k ? e2f<DT>(f2e<DT>(y[i])) : y[i];
    if (!__builtin_isfinite(v)) v = 0.f;
    y[i] = v;
    amax = fmaxf(amax, fabsf(v));
  }
  amax = wave_max(amax);
  const float scale = amax > 0.f ? amax / 448.f : 1.f;  // IEEE division (hipcc's default): torch's bits
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fminf(fmaxf(y[i] / scale, -448.f), 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  const int hk = is_k ? j - H : j - H - Hkv;
  long long boff, soff;
  kv8_row(tbl, tbl_stride, ps_shift, slots[b], p, cs_slot, cs_pos, ss_slot, boff, soff);
  if (act) *reinterpret_cast<int*>((is_k ? kc : vc) + boff + hk * cs_head + d0) = w;
  if (lane == 0) (is_k ? ks : vs)[soff + hk * ss_head] = scale;
}

KCA_API int kca_kv8_prep(void* qkv, long long ld, int B, int H, int Hkv, int D, int rot, int interleaved,
                         const float* cos_t, const float* sin_t, const int* pos, const int* slots, void* kc,
                         void* vc, float* ks, float* vs, long long cs_slot, long long cs_head, long long cs_pos,
                         long long ss_slot, long long ss_head, const int* tbl, int tbl_stride, int ps_shift, int dt,
                         hipStream_t stream) {
  if (D <= 0 || D % 8 || D > 256 || rot < 0 || rot > D || (rot & 1) || B <= 0 || H <= 0 || Hkv <= 0) return 1;
  if (rot > 0 && (!cos_t || !sin_t)) return 8;
  if (tbl && (ps_shift < 4 || ps_shift > 20 || tbl_stride <= 0)) return 5;
  if (dt != 0 && dt != 1) return 2;
  if ((cs_pos | cs_head | cs_slot) % 4) return 1;  // a lane's four bytes are one aligned 32-bit store
  const long long rows = (long long)B * (H + 2 * Hkv);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dt == 1)
    hipLaunchKernelGGL((kv8_prep_kernel<1>), grid, dim3(256), 0, stream, (uint16_t*)qkv, ld, B, H, Hkv, D, rot,
                       interleaved, cos_t, sin_t, pos, slots, (uint8_t*)kc, (uint8_t*)vc, ks, vs, cs_slot, cs_head,
                       cs_pos, ss_slot, ss_head, tbl, tbl_stride, ps_shift);
  else
    hipLaunchKernelGGL((kv8_prep_kernel<0>), grid, dim3(256), 0, stream, (uint16_t*)qkv, ld, B, H, Hkv, D, rot,
                       interleaved, cos_t, sin_t, pos, slots, (uint8_t*)kc, (uint8_t*)vc, ks, vs, cs_slot, cs_head,
                       cs_pos, ss_slot, ss_head, tbl, tbl_stride, ps_shift);
  return 0;
}

// ------------------------------------------------------------- attention
struct Kv8Params {
  const uint16_t* q;
  long long q_bs;  // q[b*q_bs + h*D + d]
  const uint8_t* kc;
  const uint8_t* vc;
  const float* ks;
  const float* vs;
  long long cs_slot, cs_head, cs_pos, ss_slot, ss_head;
  const int* slots;
  const int* kv_lens;
  uint16_t* out;
  long long o_bs;
  float* ws_o;   // [B*H, nsplit, D]
  float* ws_ml;  // [B*H, nsplit, 2]
  const float* alibi;
  const int* tbl;
  int tbl_stride, ps_shift;
  int H, Hkv, D, chunk, max_kv, window;
  float scale;
};

template <int CTRL>
__device__ __forceinline__ float kv8_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
// sum over the LPT consecutive lanes of a lane group, the result in every lane of it (decode.hip group_sum)
template <int LPT>
__device__ __forceinline__ float kv8_group_sum(float v) {
  v += kv8_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += kv8_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += kv8_dpp<0x141>(v);  // row_half_mirror
  if constexpr (LPT > 8) v += kv8_dpp<0x140>(v);  // row_mirror
  if constexpr (LPT > 16) v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));
  return v;
}

// eight e4m3 bytes -> fp32 (v_cvt_pk_f32_fp8, two per instruction; exact)
typedef float kv8_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void kv8_cvt8(const uint2 w, float (&x)[8]) {
  const kv8_f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
  const kv8_f2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
  x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  x[4] = c.x; x[5] = c.y; x[6] = d.x; x[7] = d.y;
}

// Workgroup (split, kv-head, sequence): LPT lanes share a token row, TPW = 64 / LPT rows per wave step,
// G query heads share each row. One pass with an online softmax per lane group. Only tokens of
// [max(c0, L - window), min(c0 + chunk, L)) are ever read: a lane past the range re-reads the range's
// last row and its weight is exp(-inf) = 0, so bytes and scales outside the range (NaN or not) cannot
// reach the result.
template <int LPT, int G, bool PAGED, int DT>
__global__ __launch_bounds__(256) void kv8_attn_kernel(Kv8Params p) {
  constexpr int TPW = 64 / LPT;
  constexpr int TPB = 4 * TPW;
  constexpr int U = 4;
  extern __shared__ float smem[];
  __shared__ int pg[1024 / 16 + 2];
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z, nsplit = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = p.D, ND = D >> 3;
  const int dslot = lane % LPT, tsub = lane / LPT;
  const bool dact = dslot < ND;
  const long long bh0 = (long long)b * p.H + hk * G;
  const int c0 = split * p.chunk;
  int L = min(p.kv_lens[b], p.max_kv);
  if constexpr (PAGED) L = (int)min((long long)L, (long long)p.tbl_stride << p.ps_shift);  // inside the table row
  const int seq = p.slots[b];
  const int pg0 = c0 >> p.ps_shift;
  if constexpr (PAGED) {  // this split's page ids, staged once (chunk <= 1024 tokens, pages >= 16 tokens)
    const int npg = min(((c0 + p.chunk - 1) >> p.ps_shift) - pg0 + 1, p.tbl_stride - pg0);
    for (int i = tid; i < npg; i += 256) pg[i] = p.tbl[(long long)seq * p.tbl_stride + pg0 + i];
  }
  const int c1 = min(c0 + p.chunk, L);
  const int ca = p.window > 0 ? max(c0, L - p.window) : c0;
  if (ca >= c1) {  // empty split (block-uniform): nothing read
    if (nsplit > 1) {
      if (tid < G) {
        p.ws_ml[((bh0 + tid) * nsplit + split) * 2] = -INFINITY;
        p.ws_ml[((bh0 + tid) * nsplit + split) * 2 + 1] = 0.f;
      }
    } else {
      for (int idx = tid; idx < G * D; idx += 256) p.out[b * p.o_bs + (long long)hk * G * D + idx] = (uint16_t)f2e<DT>(0.f);
    }
    return;
  }
  float q[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (dact) {
      load8_t<DT>(p.q + b * p.q_bs + (long long)(hk * G + g) * D + dslot * 8, q[g]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) q[g][j] = 0.f;
    }
  }
  float slope[G];
#pragma unroll
  for (int g = 0; g < G; ++g) slope[g] = p.alibi ? p.alibi[hk * G + g] : 0.f;
  if constexpr (PAGED) __syncthreads();  // pg[] published
  // inactive lanes (dslot >= ND) read dims [0, 8) of an in-range row instead of branching around the loads
  const long long hoff = hk * p.cs_head + (dact ? dslot * 8 : 0);
  const uint8_t* kb = p.kc + hoff;
  const uint8_t* vb = p.vc + hoff;
  const float* ksb = p.ks + hk * p.ss_head;
  const float* vsb = p.vs + hk * p.ss_head;
  auto toff = [&](int t, long long& bo, long long& so) {
    if constexpr (PAGED) {
      const long long page = pg[(t >> p.ps_shift) - pg0];
      const int tt = t & ((1 << p.ps_shift) - 1);
      bo = page * p.cs_slot + (long long)tt * p.cs_pos;
      so = page * p.ss_slot + tt;
    } else {
      bo = (long long)seq * p.cs_slot + (long long)t * p.cs_pos;
      so = (long long)seq * p.ss_slot + t;
    }
  };

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
  }
  for (int t0 = ca + wid * TPW + tsub; t0 < c1; t0 += TPB * U) {
    uint2 kk[U], vv[U];
    float sk[U], svv[U];
    long long bo[U], so[U];
#pragma unroll
    for (int u = 0; u < U; ++u) toff(min(t0 + u * TPB, c1 - 1), bo[u], so[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {  // 2U row loads + the rows' scales in flight together
      kk[u] = *reinterpret_cast<const uint2*>(kb + bo[u]);
      vv[u] = *reinterpret_cast<const uint2*>(vb + bo[u]);
      sk[u] = ksb[so[u]];
      svv[u] = vsb[so[u]];
    }
    // the U scores are independent; ONE online-softmax update folds them in. Token t0 (u = 0) is
    // always in range, so the running max is finite.
    float sv[G][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * TPB;
      float kf[8];
      kv8_cvt8(kk[u], kf);
      const float rs = p.scale * sk[u];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(q[g][j], kf[j], d);  // q == 0 on inactive lanes
        d = kv8_group_sum<LPT>(d);
        sv[g][u] = t < c1 ? fmaf(rs, d, slope[g] * (float)(t - (L - 1))) : -INFINITY;
      }
    }
    float pw[G][U];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = sv[g][0];
#pragma unroll
      for (int u = 1; u < U; ++u) mx = fmaxf(mx, sv[g][u]);
      const float mn = fmaxf(m[g], mx);
      const float cs = __expf(m[g] - mn);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float pu = __expf(sv[g][u] - mn);  // 0 for tokens past the range
        ps += pu;
        pw[g][u] = pu * svv[u];  // (a re-read in-range row's scale: finite)
      }
      l[g] = l[g] * cs + ps;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= cs;
      m[g] = mn;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      kv8_cvt8(vv[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = fmaf(pw[g][u], vf[j], acc[g][j]);
    }
  }

  // merge the lane groups: the TPW groups of a wave by shuffles, the 4 waves through LDS
#pragma unroll
  for (int o = LPT; o < 64; o <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mo = __shfl_xor(m[g], o, 64), lo = __shfl_xor(l[g], o, 64);
      const float M = fmaxf(m[g], mo);
      const float wa = m[g] == -INFINITY ? 0.f : __expf(m[g] - M);
      const float wb = mo == -INFINITY ? 0.f : __expf(mo - M);
      l[g] = l[g] * wa + lo * wb;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] = acc[g][j] * wa + __shfl_xor(acc[g][j], o, 64) * wb;
      m[g] = M;
    }
  }
  float* gm = smem;          // [4][G]
  float* gl = gm + 4 * G;    // [4][G]
  float* gacc = gl + 4 * G;  // [4][G][D]
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      gm[wid * G + g] = m[g];
      gl[wid * G + g] = l[g];
    }
  }
  if (tsub == 0 && dact) {
#pragma unroll
    for (int g = 0; g < G; ++g) store8f(gacc + (long long)(wid * G + g) * D + dslot * 8, acc[g]);
  }
  __syncthreads();
  for (int idx = tid; idx < G * D; idx += 256) {
    const int g = idx / D, d = idx % D;
    float M = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) M = fmaxf(M, gm[r * G + g]);
    float Ls = 0.f, O = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mr = gm[r * G + g];
      const float w = mr == -INFINITY ? 0.f : __expf(mr - M);
      Ls = fmaf(w, gl[r * G + g], Ls);
      O = fmaf(w, gacc[(r * G + g) * D + d], O);
    }
    if (nsplit == 1) {
      p.out[b * p.o_bs + (long long)(hk * G + g) * D + d] = (uint16_t)f2e<DT>(Ls > 0.f ? O / Ls : 0.f);
    } else {
      p.ws_o[((bh0 + g) * nsplit + split) * D + d] = O;
      if (d == 0) {
        p.ws_ml[((bh0 + g) * nsplit + split) * 2] = M;
        p.ws_ml[((bh0 + g) * nsplit + split) * 2 + 1] = Ls;
      }
    }
  }
}

// One workgroup per (sequence, head): the split weights in one pass into LDS, then every lane owns one
// output dim and adds the splits in split order (decode.hip decode_combine_kernel).
template <int DT>
__global__ __launch_bounds__(256) void kv8_combine_kernel(const float* __restrict__ ws_o,
                                                          const float* __restrict__ ws_ml,
                                                          uint16_t* __restrict__ out, long long o_bs, int H, int D,
                                                          int nsplit) {
  __shared__ float wsp[1024];
  __shared__ float red[8];
  const long long bh = blockIdx.x;
  const int b = (int)(bh / H), h = (int)(bh % H);
  const int tid = threadIdx.x;
  const float* ml = ws_ml + bh * nsplit * 2;
  const float* o = ws_o + bh * nsplit * D;
  float m = -INFINITY;
  for (int s = tid; s < nsplit; s += 256) m = fmaxf(m, ml[2 * s]);
  const float M = block_max(m, red);
  float l = 0.f;
  for (int s = tid; s < nsplit; s += 256) {
    const float ms = ml[2 * s];
    const float w = ms == -INFINITY ? 0.f : __expf(ms - M);
    wsp[s] = w;
    l += w * ml[2 * s + 1];
  }
  const float Lsum = block_sum(l, red + 4);  // block_sum's barriers also publish wsp
  const float inv = Lsum > 0.f ? 1.f / Lsum : 0.f;
  if (tid < D) {  // D <= 256: one output dim per lane
    float acc = 0.f;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {  // an empty split's partial was never written: selected out
      const float ov = o[(long long)s * D + tid];
      acc = wsp[s] > 0.f ? fmaf(wsp[s], ov, acc) : acc;
    }
    out[b * o_bs + (long long)h * D + tid] = (uint16_t)f2e<DT>(acc * inv);
  }
}

template <int LPT, int G, int DT>
static void kv8_launch(const Kv8Params& p, int B, int nsplit, hipStream_t stream) {
  const dim3 grid(nsplit, p.Hkv, B);
  const size_t lds = (size_t)4 * G * (2 + p.D) * sizeof(float);
  if (p.tbl) hipLaunchKernelGGL((kv8_attn_kernel<LPT, G, true, DT>), grid, dim3(256), lds, stream, p);
  else hipLaunchKernelGGL((kv8_attn_kernel<LPT, G, false, DT>), grid, dim3(256), lds, stream, p);
}

template <int LPT, int DT>
static void kv8_launch_g(const Kv8Params& p, int G, int B, int nsplit, hipStream_t s) {
  switch (G) {
    case 1: kv8_launch<LPT, 1, DT>(p, B, nsplit, s); break;
    case 2: kv8_launch<LPT, 2, DT>(p, B, nsplit, s); break;
    case 4: kv8_launch<LPT, 4, DT>(p, B, nsplit, s); break;
    default: kv8_launch<LPT, 8, DT>(p, B, nsplit, s); break;
  }
}

template <int DT>
static void kv8_launch_d(const Kv8Params& p, int G, int B, int nsplit, hipStream_t s) {
  const int nd = p.D / 8;
  if (nd <= 8) kv8_launch_g<8, DT>(p, G, B, nsplit, s);
  else if (nd <= 16) kv8_launch_g<16, DT>(p, G, B, nsplit, s);
  else kv8_launch_g<32, DT>(p, G, B, nsplit, s);
}

// The workspace is the 16-bit kernel's (ops/decode.py decode_ws_floats): its first B*H words (padded
// to 16 B; that kernel's fan-in counters) are left untouched, the partials follow.
KCA_API int kca_kv8_attn(const void* q, long long q_bs, const void* kc, const void* vc, const float* ks,
                         const float* vs, long long cs_slot, long long cs_head, long long cs_pos, long long ss_slot,
                         long long ss_head, const int* slots, const int* kv_lens, void* out, long long o_bs,
                         float* ws, long long ws_floats, int B, int H, int Hkv, int D, int max_kv, int chunk,
                         float scale, const float* alibi, const int* tbl, int tbl_stride, int ps_shift, int window,
                         int dt, hipStream_t stream) {
  if (D <= 0 || D % 8 || D > 256 || H <= 0 || Hkv <= 0 || H % Hkv || B <= 0 || max_kv <= 0) return 1;
  if (dt != 0 && dt != 1) return 2;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return 3;
  if (window < 0) return 9;
  if (tbl && (ps_shift < 4 || ps_shift > 20 || tbl_stride <= 0)) return 5;  // pages of >= 16 tokens
  if ((cs_pos | cs_head | cs_slot) % 8) return 1;  // a lane's eight bytes are one aligned 64-bit load
  if (chunk <= 0) chunk = kca_decode_chunk(B, Hkv, max_kv);
  if (tbl && chunk > 1024) return 6;  // the LDS page-id stage holds 1024 tokens of pages
  const int nsplit = (max_kv + chunk - 1) / chunk;
  if (nsplit > 1024) return 7;  // the combine keeps the split weights in LDS
  Kv8Params p{(const uint16_t*)q, q_bs, (const uint8_t*)kc, (const uint8_t*)vc, ks, vs, cs_slot, cs_head, cs_pos,
              ss_slot, ss_head, slots, kv_lens, (uint16_t*)out, o_bs, nullptr, nullptr, alibi, tbl, tbl_stride,
              ps_shift, H, Hkv, D, chunk, max_kv, window, scale};
  if (nsplit > 1) {
    const long long cw = ((long long)B * H + 3) / 4 * 4;
    const long long need = cw + (long long)B * H * nsplit * (D + 2);
    if (!ws || ws_floats < need) return 4;
    p.ws_o = ws + cw;
    p.ws_ml = p.ws_o + (long long)B * H * nsplit * D;
  }
  if (dt == 1) kv8_launch_d<1>(p, G, B, nsplit, stream);
  else kv8_launch_d<0>(p, G, B, nsplit, stream);
  if (nsplit > 1) {
    if (dt == 1)
      hipLaunchKernelGGL((kv8_combine_kernel<1>), dim3(B * H), dim3(256), 0, stream, p.ws_o, p.ws_ml, p.out, p.o_bs,
                         H, D, nsplit);
    else
      hipLaunchKernelGGL((kv8_combine_kernel<0>), dim3(B * H), dim3(256), 0, stream, p.ws_o, p.ws_ml, p.out, p.o_bs,
                         H, D, nsplit);
  }
  return 0;
}
