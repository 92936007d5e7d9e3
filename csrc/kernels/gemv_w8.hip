// FP8 weight-only decode linears: y[M, N] = act(scale[n] * (x[M, K] . Wq[N, K]^T) + bias[n]), M = 1..64.
//
// Wq holds OCP e4m3fn bytes (gfx950's native fp8; not the fnuz encoding of gfx942), one fp32 scale per
// output row (ops/w8.py quantize_weight). Weight-only: the activation, the accumulation (fp32) and the
// output stay what the 16-bit kernels use, so a decode step streams half the weight bytes and nothing
// else changes. e4m3 is exactly representable in bf16 and fp16, so the in-register conversion
// (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0, two elements per instruction) is exact and the
// products are the ones ops/w8.py w8_linear_reference forms; the row scale multiplies the fp32 sum in
// the epilogue, then bias, then the activation, then ONE rounding to the element type.
//
// Two kernels, both with every output element owned by one wave and its K loop in a fixed order -- no
// split-K over workgroups, no workspace, no atomics: the same call gives the same bits (seeded sampling
// replays under HIP graphs):
//
//   * M = 1..4 (w8_gemv_kernel): a wave owns W8_R = 4 weight rows, its lanes split K in 16-element
//     pieces: one 16-B non-temporal load per row and piece (two pieces in flight per row), converted to
//     packed 16-bit pairs and accumulated with v_dot2 (fp32) against the rows of x, which every wave
//     re-reads from L1 / L2 (2 M bytes per 4 weight bytes). Wave reduction, epilogue, scalar stores.
//   * M = 5..64 (w8_mfma_kernel): v_mfma_f32_16x16x32_{bf16,f16}. The weight needs no LDS transpose: a
//     lane loads 16 consecutive e4m3 of row (lane & 15) at K offset 16 * (lane >> 4) of a 64-wide K run
//     -- the first 8 bytes are its A fragment of one MFMA step, the last 8 of the next -- and the
//     activation fragment of the same lane is read from the matching K offsets, so the K order inside
//     a step pair is permuted identically on both operands. A workgroup owns 64 weight rows: KG groups
//     of 4 waves; the waves of a group split the rows and share each 128-wide K chunk of x through the
//     group's LDS stage (double-buffered, 16-B pieces XOR-swizzled by row as in skinny_mfma.hip); the
//     groups take the chunks round-robin, so a workgroup keeps KG chunks' loads in flight and its
//     serial chain is K / (128 KG) iterations (with one group and one chunk of prefetch a K = 16384
//     projection ran 128 dependent memory round trips: 95 us against 33 us for the bf16 kernel).
//     Weights and activation rows are requested two iterations ahead (register rings of three). The
//     groups' partial tiles are summed through LDS by group 0 in group order, then the epilogue.
#include "common.h"

typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// two e4m3 bytes (low or high half of `w`) -> a packed pair of the element type, exact
template <int DT, bool HI>
__device__ __forceinline__ uint32_t w8_cvt2(uint32_t w) {
  if constexpr (DT == 0) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
}

__device__ __forceinline__ u32x4v w8_ld_nt16(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4v*>(p));
}

template <int DT>
__device__ __forceinline__ float w8_epilogue(float acc, float scale, const uint16_t* bias, int n, int act) {
  float o = scale * acc;
  if (bias) o += e2f<DT>(bias[n]);
  if (act == 1) o = gelu_tanh(o);
  else if (act == 2) o = 0.5f * o * (1.f + erff(o * 0.70710678118654752f));
  return o;
}

// ---------------------------------------------------------------------------------------- M = 1..4
constexpr int W8_R = 4;   // weight rows per wave
constexpr int W8_WV = 4;  // waves per workgroup

template <int DT, int MP>
__global__ __launch_bounds__(W8_WV * 64) void w8_gemv_kernel(const uint16_t* __restrict__ x, long long ldx,
                                                             const uint8_t* __restrict__ wq,
                                                             const float* __restrict__ scale,
                                                             const uint16_t* __restrict__ bias,
                                                             uint16_t* __restrict__ y, long long ldy, int M, int N,
                                                             int K, int act) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * W8_WV + wv) * W8_R;
  if (n0 >= N) return;  // (wave-uniform; the kernel has no barrier)
  const int np = K >> 4;  // 16-element pieces per row
  const uint8_t* wr[W8_R];
#pragma unroll
  for (int r = 0; r < W8_R; ++r) wr[r] = wq + (long long)min(n0 + r, N - 1) * K;  // rows past N: a valid row, never stored
  float acc[W8_R][MP];
#pragma unroll
  for (int r = 0; r < W8_R; ++r)
#pragma unroll
    for (int m = 0; m < MP; ++m) acc[r][m] = 0.f;

  for (int p0 = lane; p0 < np; p0 += 128) {
    u32x4v w[2][W8_R], xv[2][MP][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = p0 + 64 * u;
      const bool ok = p < np;
#pragma unroll
      for (int r = 0; r < W8_R; ++r) w[u][r] = ok ? w8_ld_nt16(wr[r] + ((long long)p << 4)) : u32x4v{0u, 0u, 0u, 0u};
#pragma unroll
      for (int m = 0; m < MP; ++m) {
        const bool xo = ok && m < M;
        const uint16_t* xp = x + (long long)m * ldx + ((long long)p << 4);
        xv[u][m][0] = xo ? *reinterpret_cast<const u32x4v*>(xp) : u32x4v{0u, 0u, 0u, 0u};
        xv[u][m][1] = xo ? *reinterpret_cast<const u32x4v*>(xp + 8) : u32x4v{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < W8_R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // word j: elements 4j .. 4j+3 of the piece
          const uint32_t lo = w8_cvt2<DT, false>(w[u][r][j]), hi = w8_cvt2<DT, true>(w[u][r][j]);
#pragma unroll
          for (int m = 0; m < MP; ++m) {
            const uint32_t x0 = xv[u][m][j >> 1][(2 * j) & 3], x1 = xv[u][m][j >> 1][((2 * j) & 3) + 1];
            acc[r][m] = dot2_acc<DT>(lo, x0, acc[r][m]);
            acc[r][m] = dot2_acc<DT>(hi, x1, acc[r][m]);
          }
        }
  }
  // wave reduction; lane r * MP + m finishes element (n0 + r, m)
  float mine = 0.f;
#pragma unroll
  for (int r = 0; r < W8_R; ++r)
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      const float s = wave_sum(acc[r][m]);
      if (lane == r * MP + m) mine = s;
    }
  if (lane < W8_R * MP) {
    const int n = n0 + lane / MP, m = lane % MP;
    if (n < N && m < M) y[(long long)m * ldy + n] = (uint16_t)f2e<DT>(w8_epilogue<DT>(mine, scale[n], bias, n, act));
  }
}

// --------------------------------------------------------------------------------------- M = 5..64
constexpr int W8_KC = 128;   // K per chunk: 16 pieces of 8 activation elements per row (the swizzle's span)
constexpr int W8_MWV = 4;    // waves per K group: 64 weight rows per workgroup
constexpr int W8_ROWS = W8_MWV * 16;

template <int DT>
__device__ __forceinline__ f32x4 w8_mfma(const u32x4v& a, const u32x4v& b, const f32x4& c) {
  if constexpr (DT == 0)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                  0, 0);
}

// MT 16-row activation tiles, KG K groups of W8_MWV waves
template <int DT, int MT, int KG>
__global__ __launch_bounds__(KG * W8_MWV * 64) void w8_mfma_kernel(const uint16_t* __restrict__ x, long long ldx,
                                                                   const uint8_t* __restrict__ wq,
                                                                   const float* __restrict__ scale,
                                                                   const uint16_t* __restrict__ bias,
                                                                   uint16_t* __restrict__ y, long long ldy, int M,
                                                                   int N, int K, int act, int vec) {
  constexpr int KC = W8_KC, GT = W8_MWV * 64;  // threads per group
  constexpr int XP = (MT * 16 * 16) / GT;      // activation pieces per thread per chunk
  constexpr int XS = MT * 16 * KC;             // one stage (elements)
  static_assert((MT * 16 * 16) % GT == 0 && GT % 16 == 0, "a thread's pieces share one column");
  static_assert(KG * 2 * XS * 2 <= 65536, "static LDS");
  static_assert((KG - 1) * W8_MWV * MT * 64 * 16 <= KG * 2 * XS * 2, "the fan-in tiles reuse the stages");
  __shared__ __attribute__((aligned(16))) uint16_t xs[KG * 2 * XS];
  const int grp = threadIdx.x / GT, gt = threadIdx.x % GT;
  const int lane = gt & 63, wv = gt >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int nw0 = blockIdx.x * W8_ROWS + wv * 16;  // this wave's first weight row
  const int nc = (K + KC - 1) / KC;
  const int nit = (nc + KG - 1) / KG;  // iterations; group grp takes chunk it * KG + grp (past nc: all zero)
  const int xp = gt & 15;
  uint16_t* xg = xs + grp * 2 * XS;
  const uint8_t* wrow = wq + (long long)min(nw0 + r16, N - 1) * K;  // rows past N: a valid row, never stored

  // weight: 16 e4m3 of row r16 at K offset 64 j + 16 g of the chunk
  auto load_w = [&](int it, u32x4v (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = (it * KG + grp) * KC + 64 * j + 16 * g;
      w[j] = k < K ? w8_ld_nt16(wrow + k) : u32x4v{0u, 0u, 0u, 0u};
    }
  };
  // activation: piece q = gt + GT i of the group's [MT*16][16] stage, row q / 16, column piece gt & 15
  auto load_x = [&](int it, u32x4v (&xr)[XP]) {
    const int k = (it * KG + grp) * KC + xp * 8;
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int m = (gt + GT * i) >> 4;
      xr[i] = (m < M && k < K) ? *reinterpret_cast<const u32x4v*>(x + (long long)m * ldx + k) : u32x4v{0u, 0u, 0u, 0u};
    }
  };
  auto store_x = [&](const u32x4v (&xr)[XP], int buf) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int m = (gt + GT * i) >> 4;
      *reinterpret_cast<u32x4v*>(xg + buf * XS + m * KC + ((xp ^ (m & 15)) << 3)) = xr[i];
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // iteration `it` (workgroup-uniform): request it + 2, run the MFMAs of it, stage it + 1 (requested one
  // iteration ago) for the next iteration
  auto step = [&](int it, const u32x4v (&wc)[2], u32x4v (&w2)[2], const u32x4v (&x1)[XP], u32x4v (&x2)[XP]) {
    if (it >= nit) return;
    const int buf = it & 1;
    if (it + 2 < nit) {
      load_w(it + 2, w2);
      load_x(it + 2, x2);
    }
    const uint16_t* xb = xg + buf * XS;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int piece = 8 * j + 2 * g + s;  // K offset 64 j + 16 g + 8 s of the chunk, on both operands
        const uint32_t w0 = wc[j][2 * s], w1 = wc[j][2 * s + 1];
        const u32x4v af = {w8_cvt2<DT, false>(w0), w8_cvt2<DT, true>(w0), w8_cvt2<DT, false>(w1),
                           w8_cvt2<DT, true>(w1)};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const u32x4v bf = *reinterpret_cast<const u32x4v*>(xb + (mt * 16 + r16) * KC + ((piece ^ r16) << 3));
          acc[mt] = w8_mfma<DT>(af, bf, acc[mt]);
        }
      }
    if (it + 1 < nit) store_x(x1, buf ^ 1);
    __syncthreads();
  };
  u32x4v W0[2], W1[2], W2[2], X0[XP], X1[XP], X2[XP];
  load_w(0, W0);
  load_x(0, X0);
  load_w(1, W1);  // (past the last chunk: zeros, nothing read)
  load_x(1, X1);
  store_x(X0, 0);
  __syncthreads();
  for (int it = 0; it < nit; it += 3) {  // ring slot = iteration % 3
    step(it, W0, W2, X1, X2);
    step(it + 1, W1, W0, X2, X0);
    step(it + 2, W2, W1, X0, X1);
  }

  // fan-in: groups 1 .. KG-1 publish their tiles through LDS (the stages are free after the last
  // barrier), group 0 adds them in group order
  if constexpr (KG > 1) {
    f32x4* red = reinterpret_cast<f32x4*>(xs);  // [KG-1][W8_MWV][MT][64]
    if (grp > 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[(((grp - 1) * W8_MWV + wv) * MT + mt) * 64 + lane] = acc[mt];
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int q = 0; q < KG - 1; ++q)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] += red[((q * W8_MWV + wv) * MT + mt) * 64 + lane];
  }

  // a finished tile: weight rows nw0 + 4 g + i (i < 4), activation row mt * 16 + r16
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int n = nw0 + 4 * g, m = mt * 16 + r16;
    if (m >= M || n >= N) continue;
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      q[i] = n + i < N ? f2e<DT>(w8_epilogue<DT>(acc[mt][i], scale[n + i], bias, n + i, act)) : 0u;
    uint16_t* d = y + (long long)m * ldy + n;
    if (vec && n + 3 < N) {
      *reinterpret_cast<uint2*>(d) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < N) d[i] = (uint16_t)q[i];
    }
  }
}

// launch-shape knob (same-box A/B): 1 forces one K group per workgroup (0: built-in choice)
static int g_w8_kgroups = 0;
KCA_API int kca_w8_set_kgroups(int kg) {
  g_w8_kgroups = kg == 1 ? 1 : 0;
  return 0;
}

// KGMAX K groups (what 64 KB of static LDS and 1024 threads allow for MT) once every group gets at
// least two chunks and the launch has at most one workgroup per CU: a CU holds one workgroup of 16
// waves, so NeoX's 288 / 384 of them ran as two rounds on the 256 CUs (QKV at M = 8: 53.5 us against
// 49.5 with one group, where several small workgroups share a CU). A shorter K runs one group too.
template <int DT, int MT, int KGMAX>
static void w8_mfma_go(const uint16_t* x, long long ldx, const uint8_t* wq, const float* scale, const uint16_t* bias,
                       uint16_t* y, long long ldy, int M, int N, int K, int act, hipStream_t s) {
  const int vec = (ldy % 4 == 0 && ((uintptr_t)y & 7) == 0) ? 1 : 0;
  const dim3 grid((N + W8_ROWS - 1) / W8_ROWS);
  const int nc = (K + W8_KC - 1) / W8_KC;
  if (nc >= 2 * KGMAX && grid.x <= 256 && g_w8_kgroups != 1)
    hipLaunchKernelGGL((w8_mfma_kernel<DT, MT, KGMAX>), grid, dim3(KGMAX * W8_MWV * 64), 0, s, x, ldx, wq, scale,
                       bias, y, ldy, M, N, K, act, vec);
  else
    hipLaunchKernelGGL((w8_mfma_kernel<DT, MT, 1>), grid, dim3(W8_MWV * 64), 0, s, x, ldx, wq, scale, bias, y, ldy, M,
                       N, K, act, vec);
}

template <int DT>
static void w8_go(const uint16_t* x, long long ldx, const uint8_t* wq, const float* scale, const uint16_t* bias,
                  uint16_t* y, long long ldy, int M, int N, int K, int act, hipStream_t s) {
  if (M <= 4) {
    const dim3 grid((N + W8_WV * W8_R - 1) / (W8_WV * W8_R)), block(W8_WV * 64);
    if (M == 1)
      hipLaunchKernelGGL((w8_gemv_kernel<DT, 1>), grid, block, 0, s, x, ldx, wq, scale, bias, y, ldy, M, N, K, act);
    else if (M == 2)
      hipLaunchKernelGGL((w8_gemv_kernel<DT, 2>), grid, block, 0, s, x, ldx, wq, scale, bias, y, ldy, M, N, K, act);
    else
      hipLaunchKernelGGL((w8_gemv_kernel<DT, 4>), grid, block, 0, s, x, ldx, wq, scale, bias, y, ldy, M, N, K, act);
  } else if (M <= 16) {
    w8_mfma_go<DT, 1, 4>(x, ldx, wq, scale, bias, y, ldy, M, N, K, act, s);
  } else if (M <= 32) {
    w8_mfma_go<DT, 2, 4>(x, ldx, wq, scale, bias, y, ldy, M, N, K, act, s);
  } else {
    w8_mfma_go<DT, 4, 2>(x, ldx, wq, scale, bias, y, ldy, M, N, K, act, s);
  }
}

// x [M, K] 16-bit rows (row stride ldx elements), wq [N, K] e4m3 bytes (contiguous), scale [N] fp32,
// bias [N] of x's type (nullable), y [M, N] (row stride ldy). dt: 0 bf16, 1 fp16. Returns nonzero
// (nothing launched) for anything outside the kernels; the caller takes the reference path.
KCA_API int kca_w8_gemm(const void* x, long long ldx, const void* wq, const float* scale, const void* bias, void* y,
                        long long ldy, int M, int N, int K, int act, int dt, hipStream_t stream) {
  if (!x || !wq || !scale || !y) return 1;
  if (M < 1 || M > 64 || N < 1 || K < 16 || K % 16 || dt < 0 || dt > 1 || act < 0 || act > 2) return 1;
  if (ldx < K || ldx % 8 || ldy < N) return 2;
  if (((uintptr_t)x & 15) || ((uintptr_t)wq & 15) || ((uintptr_t)scale & 3) || ((uintptr_t)y & 1) ||
      ((uintptr_t)bias & 1))
    return 2;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint8_t* wp = static_cast<const uint8_t*>(wq);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  uint16_t* yp = static_cast<uint16_t*>(y);
  if (dt == 0) w8_go<0>(xp, ldx, wp, scale, bp, yp, ldy, M, N, K, act, stream);
  else w8_go<1>(xp, ldx, wp, scale, bp, yp, ldy, M, N, K, act, stream);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}
