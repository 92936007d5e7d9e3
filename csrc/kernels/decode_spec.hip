// Speculative decoding (draft and verify): the decode step of T tokens per sequence.
//
//   kca_spec_prep   RoPE on the Q (in place) and K of the rows [B*T, (H+2Hkv)*D] -- row b*T + t is token
//                   t of sequence b, at position base[b] + t -- and K/V of the rows t < n_tok[b] appended
//                   to the 16-bit cache. kca_decode_prep's arithmetic and lane layout row by row, so the
//                   bf16 bytes are the same; fp16 rows too (dt = 1). Rows t >= n_tok[b] write nothing.
//   kca_spec_attn   split-K decode attention in which the Q = G*T queries of one (sequence, kv-head) share
//                   every K/V row load: query t attends to positions [lo, kv_len - n_tok + t + 1), lo = 0
//                   or qpos + 1 - window; ALiBi slope * (t_key - qpos). One pass, an online softmax per
//                   lane group and query; a key past a query's limit scores -inf for that query only.
//                   Rows t >= n_tok[b] come out as zeros. Splits leave (O, max, sum) partials in the fp32
//                   workspace and spec_combine_kernel folds them in split order: no atomics, the same
//                   inputs give the same bits, and nothing in the workspace outlives a call.
//
// Cache layout and lane layout: decode.hip's / decode_kv8.hip's -- 8 dims of a row per lane, LPT = 8 / 16
// / 32 lanes per token row, 2U 16-byte row loads in flight per lane (U = 4; U = 2 at Q = 8, where q and
// the P.V accumulators alone are 128 registers). Page ids of a split are staged in LDS.
//
// Launches per layer: prep, attention, and the combine when the cache spans more than one split.
#include <algorithm>

#include "common.h"

extern "C" int kca_decode_chunk(int B, int Hkv, int max_kv);  // decode.hip: the split size

// ------------------------------------------------------------------ prep
// One wave per (row, head-row); a lane owns dims lane, lane + 64, ... (decode_prep_kernel's layout and
// expression order: the rounding is the same). Every lane loads before any lane stores.
template <int DT>
__global__ __launch_bounds__(256) void spec_prep_kernel(
    uint16_t* __restrict__ qkv, long long ld, int B, int T, int H, int Hkv, int D, int rot, int interleaved,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, const int* __restrict__ base,
    const int* __restrict__ n_tok, const int* __restrict__ slots, uint16_t* __restrict__ kc,
    uint16_t* __restrict__ vc, long long cs_slot, long long cs_head, long long cs_pos, const int* __restrict__ tbl,
    int tbl_stride, int ps_shift, int max_pos) {
  const int rows_per_b = H + 2 * Hkv;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)B * T * rows_per_b) return;
  const int lane = threadIdx.x & 63;
  const int r = (int)(row / rows_per_b), j = (int)(row % rows_per_b);
  const int b = r / T, t = r % T;
  if (t >= n_tok[b]) return;  // a padding row: nothing rotated, nothing appended
  const int p = base[b] + t;
  if (p < 0 || p >= max_pos) return;  // outside the tables and the slot's capacity: nothing written
  uint16_t* src = qkv + r * ld + (long long)j * D;
  float x[4], y[4];
  const int half = rot >> 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    x[i] = 0.f;
    y[i] = 0.f;
    if (d < D) {
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
    if (rot > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = lane + 64 * i;
        if (d < D && d < rot) src[d] = (uint16_t)f2e<DT>(y[i]);
      }
    }
    return;
  }
  const bool is_k = j < H + Hkv;
  const int hk = is_k ? j - H : j - H - Hkv;
  long long off;
  if (tbl) {
    const int page = tbl[(long long)slots[b] * tbl_stride + (p >> ps_shift)];
    KCA_DASSERT(page >= 0);
    off = (long long)page * cs_slot + (long long)(p & ((1 << ps_shift) - 1)) * cs_pos;
  } else {
    off = (long long)slots[b] * cs_slot + (long long)p * cs_pos;
  }
  uint16_t* dst = (is_k ? kc : vc) + off + hk * cs_head;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < D) dst[d] = (uint16_t)f2e<DT>(y[i]);
  }
}

// max_pos: positions the rope tables and a sequence's cache hold; a row at or past it writes nothing
KCA_API int kca_spec_prep(void* qkv, long long ld, int B, int T, int H, int Hkv, int D, int rot, int interleaved,
                          const float* cos_t, const float* sin_t, const int* base, const int* n_tok,
                          const int* slots, void* kc, void* vc, long long cs_slot, long long cs_head,
                          long long cs_pos, const int* tbl, int tbl_stride, int ps_shift, int max_pos, int dt,
                          hipStream_t stream) {
  if (D <= 0 || D > 256 || rot < 0 || rot > D || (rot & 1) || B <= 0 || T <= 0 || H <= 0 || Hkv <= 0) return 1;
  if (rot > 0 && (!cos_t || !sin_t)) return 8;
  if (tbl && (ps_shift < 0 || ps_shift > 20 || tbl_stride <= 0)) return 5;
  if (dt != 0 && dt != 1) return 2;
  if (max_pos <= 0) return 1;
  if (tbl) max_pos = (int)std::min((long long)max_pos, (long long)tbl_stride << ps_shift);
  else if (cs_pos > 0) max_pos = (int)std::min((long long)max_pos, cs_head / cs_pos);
  const long long rows = (long long)B * T * (H + 2 * Hkv);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dt == 1)
    hipLaunchKernelGGL((spec_prep_kernel<1>), grid, dim3(256), 0, stream, (uint16_t*)qkv, ld, B, T, H, Hkv, D, rot,
                       interleaved, cos_t, sin_t, base, n_tok, slots, (uint16_t*)kc, (uint16_t*)vc, cs_slot, cs_head,
                       cs_pos, tbl, tbl_stride, ps_shift, max_pos);
  else
    hipLaunchKernelGGL((spec_prep_kernel<0>), grid, dim3(256), 0, stream, (uint16_t*)qkv, ld, B, T, H, Hkv, D, rot,
                       interleaved, cos_t, sin_t, base, n_tok, slots, (uint16_t*)kc, (uint16_t*)vc, cs_slot, cs_head,
                       cs_pos, tbl, tbl_stride, ps_shift, max_pos);
  return 0;
}

// ------------------------------------------------------------- attention
struct SpecParams {
  const uint16_t* q;
  long long q_bs;  // q[(b*T + t)*q_bs + h*D + d]
  const uint16_t* kc;
  const uint16_t* vc;
  long long cs_slot, cs_head, cs_pos;
  const int* slots;
  const int* kv_lens;
  const int* n_tok;
  uint16_t* out;
  long long o_bs;
  float* ws_o;   // [B*T*H, nsplit, D]
  float* ws_ml;  // [B*T*H, nsplit, 2]
  const float* alibi;
  const int* tbl;
  int tbl_stride, ps_shift;
  int H, Hkv, D, G, T, chunk, max_kv, window;
  float scale;
};

template <int CTRL>
__device__ __forceinline__ float spec_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
// sum over the LPT consecutive lanes of a lane group, the result in every lane of it (decode.hip group_sum)
template <int LPT>
__device__ __forceinline__ float spec_group_sum(float v) {
  v += spec_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += spec_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += spec_dpp<0x141>(v);  // row_half_mirror
  if constexpr (LPT > 8) v += spec_dpp<0x140>(v);  // row_mirror
  if constexpr (LPT > 16) v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));
  return v;
}

// page ids of a split: <= 1024 tokens in pages of >= 16 tokens (+ a straddled page), padded to 16 bytes
constexpr int SPEC_PG_INTS = 1024 / 16 + 4;

// Workgroup (split, kv-head, sequence): LPT lanes share a token row, TPW = 64 / LPT rows per wave step,
// the Q = G*T queries (index t*G + g) share each row. Only tokens of [ca, c1) -- the split's part of
// [0, L), cut on the left to the oldest key the first query's window reaches -- are ever read: a lane
// past the range re-reads the range's last row with weight 0, so rows at or past L (NaN or not) cannot
// reach the result. A key inside the range but outside query qi's [lo, hi[qi]) scores -inf for qi.
template <int LPT, int Q, int U, bool PAGED, int DT>
__global__ __launch_bounds__(256) void spec_attn_kernel(SpecParams p) {
  constexpr int TPW = 64 / LPT;
  constexpr int TPB = 4 * TPW;
  // all LDS in the dynamic region (a static array in front of it would push its base off the 16-byte
  // grid the float4 accesses below need): [4][Q] max, [4][Q] sum, [4][Q][D] partial O, then the page ids
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* pg = reinterpret_cast<int*>(smem + 4 * Q * (2 + p.D));  // SPEC_PG_INTS of them (paged only)
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z, nsplit = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = p.D, ND = D >> 3, G = p.G, T = p.T;
  const int dslot = lane % LPT, tsub = lane / LPT;
  const bool dact = dslot < ND;
  const int c0 = split * p.chunk;
  int L = min(p.kv_lens[b], p.max_kv);
  if constexpr (PAGED) L = (int)min((long long)L, (long long)p.tbl_stride << p.ps_shift);  // inside the table row
  const int n = max(0, min(min(p.n_tok[b], T), L));  // rows [0, n) are tokens; the first is at L - n
  const int seq = p.slots[b];
  const int pg0 = c0 >> p.ps_shift;
  if constexpr (PAGED) {  // this split's page ids, staged once (chunk <= 1024 tokens, pages >= 16 tokens)
    const int npg = min(((c0 + p.chunk - 1) >> p.ps_shift) - pg0 + 1, p.tbl_stride - pg0);
    for (int i = tid; i < npg; i += 256) pg[i] = p.tbl[(long long)seq * p.tbl_stride + pg0 + i];
  }
  // row and head of query qi, as offsets into q / out / the workspace
  auto qrow = [&](int qi) { return (long long)b * T + qi / G; };
  auto qhead = [&](int qi) { return hk * G + qi % G; };
  const int c1 = min(c0 + p.chunk, L);
  const int ca = p.window > 0 ? max(c0, L - n + 1 - p.window) : c0;
  if (n == 0 || ca >= c1) {  // empty split (block-uniform): nothing read
    if (nsplit > 1) {
      if (tid < Q) {
        const long long bh = qrow(tid) * p.H + qhead(tid);
        p.ws_ml[(bh * nsplit + split) * 2] = -INFINITY;
        p.ws_ml[(bh * nsplit + split) * 2 + 1] = 0.f;
      }
    } else {
      for (int idx = tid; idx < Q * D; idx += 256) {
        const int qi = idx / D, d = idx % D;
        p.out[qrow(qi) * p.o_bs + (long long)qhead(qi) * D + d] = (uint16_t)f2e<DT>(0.f);
      }
    }
    return;
  }
  float q[Q][8], slope[Q];
  int hi[Q];  // query qi sees keys below hi[qi] (0: a padding row, sees nothing)
#pragma unroll
  for (int qi = 0; qi < Q; ++qi) {
    const int t = qi / G;
    hi[qi] = t < n ? L - n + t + 1 : 0;
    slope[qi] = p.alibi ? p.alibi[qhead(qi)] : 0.f;
    if (dact && t < n) {
      load8_t<DT>(p.q + qrow(qi) * p.q_bs + (long long)qhead(qi) * D + dslot * 8, q[qi]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) q[qi][j] = 0.f;
    }
  }
  if constexpr (PAGED) __syncthreads();  // pg[] published
  // inactive lanes (dslot >= ND) read dims [0, 8) of an in-range row instead of branching around the loads
  const long long hoff = hk * p.cs_head + (dact ? dslot * 8 : 0);
  const uint16_t* kb = p.kc + hoff;
  const uint16_t* vb = p.vc + hoff;
  auto toff = [&](int t) -> long long {
    if constexpr (PAGED) {
      const long long page = pg[(t >> p.ps_shift) - pg0];
      return page * p.cs_slot + (long long)(t & ((1 << p.ps_shift) - 1)) * p.cs_pos;
    } else {
      return (long long)seq * p.cs_slot + (long long)t * p.cs_pos;
    }
  };

  float m[Q], l[Q], acc[Q][8];
#pragma unroll
  for (int qi = 0; qi < Q; ++qi) {
    m[qi] = -INFINITY;
    l[qi] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[qi][j] = 0.f;
  }
  for (int t0 = ca + wid * TPW + tsub; t0 < c1; t0 += TPB * U) {
    U16x8 kk[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // 2U row loads in flight together
      const long long o = toff(min(t0 + u * TPB, c1 - 1));
      kk[u] = *reinterpret_cast<const U16x8*>(kb + o);
      vv[u] = *reinterpret_cast<const U16x8*>(vb + o);
    }
    // the U scores of a query are independent; ONE online-softmax update per query folds them in
    float sv[Q][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * TPB;
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = e2f<DT>(kk[u].v[j]);
#pragma unroll
      for (int qi = 0; qi < Q; ++qi) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(q[qi][j], kf[j], d);  // q == 0 on inactive lanes
        d = spec_group_sum<LPT>(d);
        const bool in = t < c1 && t < hi[qi] && (p.window <= 0 || t >= hi[qi] - p.window);
        sv[qi][u] = in ? fmaf(p.scale, d, slope[qi] * (float)(t - (hi[qi] - 1))) : -INFINITY;
      }
    }
    float pw[Q][U];
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) {
      float mx = sv[qi][0];
#pragma unroll
      for (int u = 1; u < U; ++u) mx = fmaxf(mx, sv[qi][u]);
      const float mn = fmaxf(m[qi], mx);
      const float mr = mn == -INFINITY ? 0.f : mn;  // no key of this query yet: every weight below is 0
      const float cs = __expf(m[qi] - mr);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pw[qi][u] = __expf(sv[qi][u] - mr);  // 0 for keys outside the query's range
        ps += pw[qi][u];
      }
      l[qi] = l[qi] * cs + ps;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[qi][j] *= cs;
      m[qi] = mn;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = e2f<DT>(vv[u].v[j]);
#pragma unroll
      for (int qi = 0; qi < Q; ++qi)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[qi][j] = fmaf(pw[qi][u], vf[j], acc[qi][j]);
    }
  }

  // merge the lane groups: the TPW groups of a wave by shuffles, the 4 waves through LDS
#pragma unroll
  for (int o = LPT; o < 64; o <<= 1) {
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) {
      const float mo = __shfl_xor(m[qi], o, 64), lo = __shfl_xor(l[qi], o, 64);
      const float M = fmaxf(m[qi], mo);
      const float wa = m[qi] == -INFINITY ? 0.f : __expf(m[qi] - M);
      const float wb = mo == -INFINITY ? 0.f : __expf(mo - M);
      l[qi] = l[qi] * wa + lo * wb;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[qi][j] = acc[qi][j] * wa + __shfl_xor(acc[qi][j], o, 64) * wb;
      m[qi] = M;
    }
  }
  float* gm = smem;          // [4][Q]
  float* gl = gm + 4 * Q;    // [4][Q]
  float* gacc = gl + 4 * Q;  // [4][Q][D]
  if (lane == 0) {
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) {
      gm[wid * Q + qi] = m[qi];
      gl[wid * Q + qi] = l[qi];
    }
  }
  if (tsub == 0 && dact) {
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) store8f(gacc + (long long)(wid * Q + qi) * D + dslot * 8, acc[qi]);
  }
  __syncthreads();
  for (int idx = tid; idx < Q * D; idx += 256) {
    const int qi = idx / D, d = idx % D;
    float M = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) M = fmaxf(M, gm[r * Q + qi]);
    float Ls = 0.f, O = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mr = gm[r * Q + qi];
      const float w = mr == -INFINITY ? 0.f : __expf(mr - M);
      Ls = fmaf(w, gl[r * Q + qi], Ls);
      O = fmaf(w, gacc[(r * Q + qi) * D + d], O);
    }
    if (nsplit == 1) {
      p.out[qrow(qi) * p.o_bs + (long long)qhead(qi) * D + d] = (uint16_t)f2e<DT>(Ls > 0.f ? O / Ls : 0.f);
    } else {
      const long long bh = qrow(qi) * p.H + qhead(qi);
      p.ws_o[(bh * nsplit + split) * D + d] = O;
      if (d == 0) {
        p.ws_ml[(bh * nsplit + split) * 2] = M;
        p.ws_ml[(bh * nsplit + split) * 2 + 1] = Ls;
      }
    }
  }
}

// One workgroup per (row, head): the split weights in one pass into LDS, then every lane owns one output
// dim and adds the splits in split order (decode_kv8.hip kv8_combine_kernel). A row with no key in any
// split (a padding row) comes out as zeros.
template <int DT>
__global__ __launch_bounds__(256) void spec_combine_kernel(const float* __restrict__ ws_o,
                                                           const float* __restrict__ ws_ml,
                                                           uint16_t* __restrict__ out, long long o_bs, int H, int D,
                                                           int nsplit) {
  __shared__ float wsp[1024];
  __shared__ float red[8];
  const long long bh = blockIdx.x;
  const long long r = bh / H;
  const int h = (int)(bh % H);
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
    out[r * o_bs + (long long)h * D + tid] = (uint16_t)f2e<DT>(acc * inv);
  }
}

template <int LPT, int Q, int DT>
static void spec_launch(const SpecParams& p, int B, int nsplit, hipStream_t stream) {
  constexpr int U = Q >= 8 ? 2 : 4;
  const dim3 grid(nsplit, p.Hkv, B);
  const size_t lds = (size_t)4 * Q * (2 + p.D) * sizeof(float);
  if (p.tbl)
    hipLaunchKernelGGL((spec_attn_kernel<LPT, Q, U, true, DT>), grid, dim3(256), lds + SPEC_PG_INTS * sizeof(int),
                       stream, p);
  else hipLaunchKernelGGL((spec_attn_kernel<LPT, Q, U, false, DT>), grid, dim3(256), lds, stream, p);
}

template <int LPT, int DT>
static void spec_launch_q(const SpecParams& p, int Q, int B, int nsplit, hipStream_t s) {
  switch (Q) {
    case 2: spec_launch<LPT, 2, DT>(p, B, nsplit, s); break;
    case 4: spec_launch<LPT, 4, DT>(p, B, nsplit, s); break;
    default: spec_launch<LPT, 8, DT>(p, B, nsplit, s); break;
  }
}

template <int DT>
static void spec_launch_d(const SpecParams& p, int Q, int B, int nsplit, hipStream_t s) {
  const int nd = p.D / 8;
  if (nd <= 8) spec_launch_q<8, DT>(p, Q, B, nsplit, s);
  else if (nd <= 16) spec_launch_q<16, DT>(p, Q, B, nsplit, s);
  else spec_launch_q<32, DT>(p, Q, B, nsplit, s);
}

// q / out rows: b*T + t. The workspace is laid out as ops/decode.py decode_ws_floats(B*T, ...): its first
// B*T*H words (padded to 16 B; the 16-bit kernel's fan-in counters) are left untouched, the partials follow.
KCA_API int kca_spec_attn(const void* q, long long q_bs, const void* kc, const void* vc, long long cs_slot,
                          long long cs_head, long long cs_pos, const int* slots, const int* kv_lens,
                          const int* n_tok, void* out, long long o_bs, float* ws, long long ws_floats, int B, int T,
                          int H, int Hkv, int D, int max_kv, int chunk, float scale, const float* alibi,
                          const int* tbl, int tbl_stride, int ps_shift, int window, int dt, hipStream_t stream) {
  if (D <= 0 || D % 8 || D > 256 || H <= 0 || Hkv <= 0 || H % Hkv || B <= 0 || T <= 0 || max_kv <= 0) return 1;
  if (dt != 0 && dt != 1) return 2;
  const int G = H / Hkv;
  const long long Q = (long long)G * T;
  if (T < 2 || (Q != 2 && Q != 4 && Q != 8)) return 3;
  if (window < 0) return 9;
  if (tbl && (ps_shift < 4 || ps_shift > 20 || tbl_stride <= 0)) return 5;  // pages of >= 16 tokens
  if ((cs_pos | cs_head | cs_slot | q_bs) % 8) return 1;  // a lane's eight elements are one aligned 16-byte load
  if (chunk <= 0) chunk = kca_decode_chunk(B, Hkv, max_kv);
  if (tbl && chunk > 1024) return 6;  // the LDS page-id stage holds 1024 tokens of pages
  const int nsplit = (max_kv + chunk - 1) / chunk;
  if (nsplit > 1024) return 7;  // the combine keeps the split weights in LDS
  SpecParams p{(const uint16_t*)q, q_bs, (const uint16_t*)kc, (const uint16_t*)vc, cs_slot, cs_head, cs_pos, slots,
               kv_lens, n_tok, (uint16_t*)out, o_bs, nullptr, nullptr, alibi, tbl, tbl_stride, ps_shift, H, Hkv, D,
               G, T, chunk, max_kv, window, scale};
  const long long rows = (long long)B * T * H;
  if (nsplit > 1) {
    const long long cw = (rows + 3) / 4 * 4;
    const long long need = cw + rows * nsplit * (D + 2);
    if (!ws || ws_floats < need) return 4;
    p.ws_o = ws + cw;
    p.ws_ml = p.ws_o + rows * nsplit * D;
  }
  if (dt == 1) spec_launch_d<1>(p, (int)Q, B, nsplit, stream);
  else spec_launch_d<0>(p, (int)Q, B, nsplit, stream);
  if (nsplit > 1) {
    if (dt == 1)
      hipLaunchKernelGGL((spec_combine_kernel<1>), dim3((unsigned)rows), dim3(256), 0, stream, p.ws_o, p.ws_ml, p.out,
                         p.o_bs, H, D, nsplit);
    else
      hipLaunchKernelGGL((spec_combine_kernel<0>), dim3((unsigned)rows), dim3(256), 0, stream, p.ws_o, p.ws_ml, p.out,
                         p.o_bs, H, D, nsplit);
  }
  return 0;
}
