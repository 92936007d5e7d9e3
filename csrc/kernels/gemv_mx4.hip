// MXFP4 weight-only decode linears: y[M, N] = act(sum_k x[m, k] v[n, k] 2^(E[n, k / 32] - 127) + bias[n]),
// M = 1..64.
//
// The weight is OCP microscaling FP4 (ops/mx4.py): wq [N, K/2] bytes, element k = 2j in the low nibble of
// byte j and k = 2j + 1 in the high one, a nibble being e2m1 (sign, 0 / 0.5 / 1 / 1.5 / 2 / 3 / 4 / 6; 0x8
// is -0 and converts to zero); wscale [N, K/32] e8m0 bytes, one per block of 32 consecutive k of a row
// (K % 32 == 0, so K tails are whole blocks). 16 bytes are one block: 0.53 bytes per weight against 2 for
// the 16-bit decode linears and 1 for gemv_w8.hip. Weight-only: activations, the fp32 accumulation and
// the output are what the 16-bit kernels use. The nibbles are converted in registers, a byte (two
// elements) per v_cvt_scalef32_pk_{bf16,f16}_fp4; every e2m1 value is a bf16 and an fp16 value, so the
// conversion is exact.
//
// Where the block scale goes. bf16 has fp32's exponent range, so in the MFMA kernel's bf16
// instantiation the scale rides in the conversion's scale operand and the scaled element is still
// exact. fp16 does not: 6 * 2^14 overflows and 0.5 * 2^-30 flushes. The fp16 MFMA instantiation
// therefore converts with scale 1, runs each block's MFMA into a zero accumulator and applies the
// scales in fp32 to the 16x16 result (four FMAs per lane: the C layout has weight row 4 (lane >> 4) +
// reg in register reg). The GEMV applies the scale in fp32 to the block's partial sum for both types.
//
// As in gemv_w8.hip every output element is finished in a fixed order -- no split-K over workgroups, no
// workspace, no atomics: the same call gives the same bits (seeded sampling replays under HIP graphs).
//
//   * M = 1..4 (mx4_gemv_kernel): a wave owns MX4_R = 4 weight rows and its lanes split K in blocks:
//     one 16-B non-temporal load per row and block (two blocks in flight per row), the block's scale
//     byte beside it (lane p reads scale[n][p]: coalesced), v_dot2 (fp32) against the rows of x, which
//     every wave re-reads from L1 / L2. Wave reduction, epilogue, scalar stores.
//   * M = 5..64 (mx4_mfma_kernel): v_mfma_f32_16x16x32_{bf16,f16}, one K step = one block. A workgroup
//     owns 16 weight rows, so that a 4096-row projection is 256 workgroups (gemv_w8.hip's 64-row
//     workgroups left three quarters of the CUs without one) -- 32 or 64 rows where N is large enough
//     that every CU still gets a workgroup (mx4_mfma_go); its MX4_KW = 8 waves split K, taking the
//     128-wide chunks (four blocks) round-robin, and their partial tiles are summed through LDS by wave 0
//     in wave order. A lane loads one whole block (16 B) of row (lane & 15), block (lane >> 4) of the
//     chunk; an MFMA step needs 8 elements of the SAME block from each of the four lanes of a row, so
//     the wave transposes the chunk through its private 1 KB of LDS (16-B pieces XOR-swizzled by row:
//     conflict-free both ways). The activation fragments come straight from global memory (the waves
//     of a workgroup read different K, nothing to share). Weights are requested two chunks ahead,
//     activations one.
#include "common.h"

typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// byte SEL of `w` (elements 2 SEL, 2 SEL + 1 of the 8 in the word) -> a packed pair of the element type,
// the low nibble's element in the low half, times `scale` (a power of two)
template <int DT, int SEL>
__device__ __forceinline__ uint32_t mx4_cvt2(uint32_t w, float scale) {
  if constexpr (DT == 0) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, SEL));
}
// the 8 elements of a word, in k order
template <int DT>
__device__ __forceinline__ u32x4v mx4_cvt8(uint32_t w, float scale) {
  return u32x4v{mx4_cvt2<DT, 0>(w, scale), mx4_cvt2<DT, 1>(w, scale), mx4_cvt2<DT, 2>(w, scale),
                mx4_cvt2<DT, 3>(w, scale)};
}

// e8m0 byte -> 2^(E - 127) (E = 0: the fp32 subnormal 2^-127)
__device__ __forceinline__ float mx4_scale(uint32_t e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }

__device__ __forceinline__ u32x4v mx4_ld_nt16(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4v*>(p));
}

template <int DT>
__device__ __forceinline__ float mx4_epilogue(float o, const uint16_t* bias, int n, int act) {
  if (bias) o += e2f<DT>(bias[n]);
  if (act == 1) o = gelu_tanh(o);
  else if (act == 2) o = 0.5f * o * (1.f + erff(o * 0.70710678118654752f));
  return o;
}

// ---------------------------------------------------------------------------------------- M = 1..4
constexpr int MX4_R = 4;   // weight rows per wave
constexpr int MX4_WV = 4;  // waves per workgroup

template <int DT, int MP>
__global__ __launch_bounds__(MX4_WV * 64) void mx4_gemv_kernel(const uint16_t* __restrict__ x, long long ldx,
                                                               const uint8_t* __restrict__ wq,
                                                               const uint8_t* __restrict__ ws,
                                                               const uint16_t* __restrict__ bias,
                                                               uint16_t* __restrict__ y, long long ldy, int M, int N,
                                                               int K, int act) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * MX4_WV + wv) * MX4_R;
  if (n0 >= N) return;  // (wave-uniform; the kernel has no barrier)
  const int nb = K >> 5;  // blocks per row
  const uint8_t* wr[MX4_R];
  const uint8_t* sr[MX4_R];
#pragma unroll
  for (int r = 0; r < MX4_R; ++r) {  // rows past N: a valid row, never stored
    const long long nr = min(n0 + r, N - 1);
    wr[r] = wq + nr * (K >> 1);
    sr[r] = ws + nr * nb;
  }
  float acc[MX4_R][MP];
#pragma unroll
  for (int r = 0; r < MX4_R; ++r)
#pragma unroll
    for (int m = 0; m < MP; ++m) acc[r][m] = 0.f;

  for (int p0 = lane; p0 < nb; p0 += 128) {
    u32x4v w[2][MX4_R];
    uint32_t e[2][MX4_R];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = p0 + 64 * u;
      const bool ok = p < nb;
#pragma unroll
      for (int r = 0; r < MX4_R; ++r) {
        w[u][r] = ok ? mx4_ld_nt16(wr[r] + ((long long)p << 4)) : u32x4v{0u, 0u, 0u, 0u};
        e[u][r] = ok ? (uint32_t)sr[r][p] : 127u;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = p0 + 64 * u;
      const bool ok = p < nb;
      u32x4v xv[MP][4];  // word j: elements 8j .. 8j+7 of the block
#pragma unroll
      for (int m = 0; m < MP; ++m) {
        const bool xo = ok && m < M;
        const uint16_t* xp = x + (long long)m * ldx + ((long long)p << 5);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xv[m][j] = xo ? *reinterpret_cast<const u32x4v*>(xp + 8 * j) : u32x4v{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int r = 0; r < MX4_R; ++r) {
        float part[MP];  // the block's sum of x * e2m1, scaled once in fp32
#pragma unroll
        for (int m = 0; m < MP; ++m) part[m] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x4v c = mx4_cvt8<DT>(w[u][r][j], 1.0f);
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int m = 0; m < MP; ++m) part[m] = dot2_acc<DT>(c[t], xv[m][j][t], part[m]);
        }
        const float s = mx4_scale(e[u][r]);
#pragma unroll
        for (int m = 0; m < MP; ++m) acc[r][m] = fmaf(s, part[m], acc[r][m]);
      }
    }
  }
  // wave reduction; lane r * MP + m finishes element (n0 + r, m)
  float mine = 0.f;
#pragma unroll
  for (int r = 0; r < MX4_R; ++r)
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      const float s = wave_sum(acc[r][m]);
      if (lane == r * MP + m) mine = s;
    }
  if (lane < MX4_R * MP) {
    const int n = n0 + lane / MP, m = lane % MP;
    if (n < N && m < M) y[(long long)m * ldy + n] = (uint16_t)f2e<DT>(mx4_epilogue<DT>(mine, bias, n, act));
  }
}

// --------------------------------------------------------------------------------------- M = 5..64
constexpr int MX4_KW = 8;        // waves per workgroup, splitting K
constexpr int MX4_ROWS = 16;     // weight rows per workgroup
constexpr int MX4_STAGE = 320;   // 32-bit words of LDS per wave: [16 rows][16] nibble words + [4 blocks][16 rows] scales

template <int DT>
__device__ __forceinline__ f32x4 mx4_mfma(const u32x4v& a, const u32x4v& b, const f32x4& c) {
  if constexpr (DT == 0)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                  0, 0);
}

// MT 16-row activation tiles, RT 16-row weight tiles per wave (16 RT weight rows per workgroup)
template <int DT, int MT, int RT>
__global__ __launch_bounds__(MX4_KW * 64) void mx4_mfma_kernel(const uint16_t* __restrict__ x, long long ldx,
                                                               const uint8_t* __restrict__ wq,
                                                               const uint8_t* __restrict__ ws,
                                                               const uint16_t* __restrict__ bias,
                                                               uint16_t* __restrict__ y, long long ldy, int M, int N,
                                                               int K, int act, int vec) {
  constexpr int RED = (MX4_KW - 1) * RT * MT * 64 * 4;  // the fan-in tiles (words); they reuse the stages
  constexpr int LDSW = RED > MX4_KW * RT * MX4_STAGE ? RED : MX4_KW * RT * MX4_STAGE;
  static_assert(LDSW * 4 <= 65536, "static LDS");
  __shared__ __attribute__((aligned(16))) uint32_t lds[LDSW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (MX4_ROWS * RT);
  const int nb = K >> 5;                         // blocks per row
  const int nc = (nb + 3) >> 2;                  // 128-wide chunks
  const int nit = (nc + MX4_KW - 1) / MX4_KW;    // iterations; wave wv takes chunk it * MX4_KW + wv
  uint32_t* wl = lds + wv * (RT * MX4_STAGE);    // tile rt: words [rt * MX4_STAGE, +256), scales behind them
  const uint8_t* wrow[RT];
  const uint8_t* srow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {  // rows past N: a valid row, never stored
    const long long nr = min(n0 + rt * 16 + r16, N - 1);
    wrow[rt] = wq + nr * (K >> 1);
    srow[rt] = ws + nr * nb;
  }
  const uint16_t* xrow[MT];  // activation rows past M: a valid row, its output column never stored
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = x + (long long)min(mt * 16 + r16, M - 1) * ldx;
  const int sw = (r16 >> 2) & 3;  // the row's swizzle of its four 16-B pieces

  // block (chunk, g) of row r16 of every tile: its 16 bytes and its scale byte. Past K: an in-range
  // address, whose bytes the consuming step replaces by zeros (a select here would wait for the load at
  // once)
  auto load_w = [&](int it, u32x4v (&w)[RT], uint32_t (&e)[RT]) {
    const int bc = min(((it * MX4_KW + wv) << 2) + g, nb - 1);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      w[rt] = mx4_ld_nt16(wrow[rt] + ((long long)bc << 4));
      e[rt] = srow[rt][bc];
    }
  };
  // the B fragments of the chunk's four blocks: row (tile, r16), elements 8g .. 8g+7 of each block. Past
  // K: an in-range address; those products meet zero weights
  auto load_x = [&](int it, u32x4v (&xr)[4][MT]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = min(((it * MX4_KW + wv) << 2) + s, nb - 1) * 32 + 8 * g;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xr[s][mt] = *reinterpret_cast<const u32x4v*>(xrow[mt] + k);
    }
  };

  f32x4 acc[RT][MT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // iteration `it` (workgroup-uniform): request the activations of it + 1 and the weights of it + 2 (past
  // the end: in-range addresses, results unused), transpose the chunk through the wave's LDS, four MFMA
  // steps per weight tile against the same activation fragments. The wave's LDS instructions execute in
  // order, so its lanes exchange data without a barrier; the wave barriers only pin the compiler's order.
  auto step = [&](int it, const u32x4v (&wc)[RT], const uint32_t (&ec)[RT], u32x4v (&w2)[RT], uint32_t (&e2)[RT],
                  const u32x4v (&xc)[4][MT], u32x4v (&x1)[4][MT]) {
    if (it >= nit) return;
    load_x(it + 1, x1);
    const bool in = ((it * MX4_KW + wv) << 2) + g < nb;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      *reinterpret_cast<u32x4v*>(wl + rt * MX4_STAGE + r16 * 16 + ((g ^ sw) << 2)) = in ? wc[rt] : u32x4v{0u, 0u, 0u, 0u};
      reinterpret_cast<float*>(wl + rt * MX4_STAGE + 256)[lane] = mx4_scale(ec[rt]);  // [block g][row r16]
    }
    load_w(it + 2, w2, e2);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const uint32_t* tl = wl + rt * MX4_STAGE;
        const float* sl = reinterpret_cast<const float*>(tl + 256);
        const uint32_t wd = tl[r16 * 16 + ((s ^ sw) << 2) + g];  // elements 8g .. 8g+7 of block s, row r16
        if constexpr (DT == 0) {
          const u32x4v af = mx4_cvt8<0>(wd, sl[s * 16 + r16]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = mx4_mfma<0>(af, xc[s][mt], acc[rt][mt]);
        } else {
          const u32x4v af = mx4_cvt8<1>(wd, 1.0f);
          const f32x4 sv = *reinterpret_cast<const f32x4*>(sl + s * 16 + 4 * g);  // rows 4g .. 4g+3: the C registers
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 t = mx4_mfma<1>(af, xc[s][mt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[rt][mt][i] = fmaf(sv[i], t[i], acc[rt][mt][i]);
          }
        }
      }
    __builtin_amdgcn_wave_barrier();
  };
  u32x4v W0[RT], W1[RT], W2[RT], X0[4][MT], X1[4][MT];
  uint32_t E0[RT], E1[RT], E2[RT];
  load_w(0, W0, E0);
  load_x(0, X0);
  load_w(1, W1, E1);
  for (int it = 0; it < nit; it += 6) {  // weight ring slot = iteration % 3, activation slot = iteration % 2
    step(it, W0, E0, W2, E2, X0, X1);
    step(it + 1, W1, E1, W0, E0, X1, X0);
    step(it + 2, W2, E2, W1, E1, X0, X1);
    step(it + 3, W0, E0, W2, E2, X1, X0);
    step(it + 4, W1, E1, W0, E0, X0, X1);
    step(it + 5, W2, E2, W1, E1, X1, X0);
  }

  // fan-in: waves 1 .. KW-1 publish their tiles through LDS (the stages are free after the barrier),
  // wave 0 adds them in wave order
  __syncthreads();
  f32x4* red = reinterpret_cast<f32x4*>(lds);  // [KW-1][RT][MT][64]
  if (wv > 0) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[(((wv - 1) * RT + rt) * MT + mt) * 64 + lane] = acc[rt][mt];
  }
  __syncthreads();
  if (wv > 0) return;
#pragma unroll
  for (int q = 0; q < MX4_KW - 1; ++q)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[rt][mt] += red[((q * RT + rt) * MT + mt) * 64 + lane];

  // a finished tile: weight rows n0 + 16 rt + 4 g + i (i < 4), activation row mt * 16 + r16
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int n = n0 + rt * 16 + 4 * g, m = mt * 16 + r16;
      if (m >= M || n >= N) continue;
      uint32_t q[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        q[i] = n + i < N ? f2e<DT>(mx4_epilogue<DT>(acc[rt][mt][i], bias, n + i, act)) : 0u;
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

// Weight tiles per wave. The activation fragments are read from L2 by every workgroup -- 64 MT bytes per
// 16-B block of one weight row, 4 MT times the weight stream with one tile -- and that traffic, not the
// weight stream, bounds the kernel (measured: docs/PERF.md Round 11). A wave that runs RT tiles against
// the same fragments divides it by RT, at 1 / RT of the workgroups: RT = 2 / 4 only where that still
// leaves every one of the 256 CUs a workgroup, RT = 4 only for M <= 16 and RT = 2 for M <= 32 (the fp16
// instantiations of MT = 2, RT = 4 and of MT = 4, RT = 2 would spill).
template <int DT, int MT>
static void mx4_mfma_go(const uint16_t* x, long long ldx, const uint8_t* wq, const uint8_t* ws, const uint16_t* bias,
                        uint16_t* y, long long ldy, int M, int N, int K, int act, hipStream_t s) {
  const int vec = (ldy % 4 == 0 && ((uintptr_t)y & 7) == 0) ? 1 : 0;
  const int tiles = (N + MX4_ROWS - 1) / MX4_ROWS;
  const dim3 block(MX4_KW * 64);
  if constexpr (MT == 1) {
    // (a grid of 288 four-tile workgroups -- NeoX's QKV -- ran as two rounds on the 256 CUs, one of these
    // workgroups fitting a CU: 44.9 us against 40.0 with one tile; whole rounds, or enough of them)
    const int wg4 = (tiles + 3) / 4;
    if (tiles >= 4 * 256 && (wg4 % 256 == 0 || wg4 >= 4 * 256)) {
      hipLaunchKernelGGL((mx4_mfma_kernel<DT, MT, 4>), dim3(wg4), block, 0, s, x, ldx, wq, ws, bias, y, ldy,
                         M, N, K, act, vec);
      return;
    }
  }
  if constexpr (MT <= 2) {
    if (tiles >= 2 * 256) {
      hipLaunchKernelGGL((mx4_mfma_kernel<DT, MT, 2>), dim3((tiles + 1) / 2), block, 0, s, x, ldx, wq, ws, bias, y, ldy,
                         M, N, K, act, vec);
      return;
    }
  }
  hipLaunchKernelGGL((mx4_mfma_kernel<DT, MT, 1>), dim3(tiles), block, 0, s, x, ldx, wq, ws, bias, y, ldy, M, N, K, act,
                     vec);
}

template <int DT>
static void mx4_go(const uint16_t* x, long long ldx, const uint8_t* wq, const uint8_t* ws, const uint16_t* bias,
                   uint16_t* y, long long ldy, int M, int N, int K, int act, hipStream_t s) {
  if (M <= 4) {
    const dim3 grid((N + MX4_WV * MX4_R - 1) / (MX4_WV * MX4_R)), block(MX4_WV * 64);
    if (M == 1)
      hipLaunchKernelGGL((mx4_gemv_kernel<DT, 1>), grid, block, 0, s, x, ldx, wq, ws, bias, y, ldy, M, N, K, act);
    else if (M == 2)
      hipLaunchKernelGGL((mx4_gemv_kernel<DT, 2>), grid, block, 0, s, x, ldx, wq, ws, bias, y, ldy, M, N, K, act);
    else
      hipLaunchKernelGGL((mx4_gemv_kernel<DT, 4>), grid, block, 0, s, x, ldx, wq, ws, bias, y, ldy, M, N, K, act);
  } else if (M <= 16) {
    mx4_mfma_go<DT, 1>(x, ldx, wq, ws, bias, y, ldy, M, N, K, act, s);
  } else if (M <= 32) {
    mx4_mfma_go<DT, 2>(x, ldx, wq, ws, bias, y, ldy, M, N, K, act, s);
  } else {
    mx4_mfma_go<DT, 4>(x, ldx, wq, ws, bias, y, ldy, M, N, K, act, s);
  }
}

// x [M, K] 16-bit rows (row stride ldx elements), wq [N, K/2] e2m1 nibble pairs (contiguous), wscale
// [N, K/32] e8m0 bytes (contiguous), bias [N] of x's type (nullable), y [M, N] (row stride ldy). dt: 0
// bf16, 1 fp16. Returns nonzero (nothing launched) for anything outside the kernels; the caller takes
// the reference path.
KCA_API int kca_mx4_gemm(const void* x, long long ldx, const void* wq, const void* wscale, const void* bias, void* y,
                         long long ldy, int M, int N, int K, int act, int dt, hipStream_t stream) {
  if (!x || !wq || !wscale || !y) return 1;
  if (M < 1 || M > 64 || N < 1 || K < 32 || K % 32 || dt < 0 || dt > 1 || act < 0 || act > 2) return 1;
  if (ldx < K || ldx % 8 || ldy < N) return 2;
  if (((uintptr_t)x & 15) || ((uintptr_t)wq & 15) || ((uintptr_t)y & 1) || ((uintptr_t)bias & 1)) return 2;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint8_t* wp = static_cast<const uint8_t*>(wq);
  const uint8_t* sp = static_cast<const uint8_t*>(wscale);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  uint16_t* yp = static_cast<uint16_t*>(y);
  if (dt == 0) mx4_go<0>(xp, ldx, wp, sp, bp, yp, ldy, M, N, K, act, stream);
  else mx4_go<1>(xp, ldx, wp, sp, bp, yp, ldy, M, N, K, act, stream);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}
