// Quantized-weight prefill GEMM: y[M, N] = act(x[M, K] . dequant(W)[N, K]^T + bias[n]) for any M >= 1
// (meant for M > 64; the decode kernels of gemv_w8.hip / gemv_mx4.hip own M <= 64).
//
//   fmt 0: W is e4m3fn bytes [N, K] plus one fp32 scale per row (ops/w8.py); K % 16 == 0. The bytes are
//          converted with scale 1.0 (exact) and the row scale multiplies the fp32 sum in the epilogue:
//          the contract is w8_linear_reference.
//   fmt 1: W is e2m1 nibbles [N, K/2] plus one e8m0 byte per 32 k (ops/mx4.py); K % 32 == 0. The
//          contract is mx4_linear_reference.
//
// fp32 accumulation, then bias, then the activation, then ONE rounding to the element type -- what the
// slab kernels do. Every output element is finished by one wave with its K loop in a fixed order: no
// split-K, no workspace, no atomics, the same call gives the same bits.
//
// A compute-bound tiled GEMM, not a weight streamer. A workgroup of 4 waves (2 along M x 2 along N)
// owns 128 rows of M x 32 RT rows of N (RT = 4: 128, RT = 2: 64 where the larger tile would leave CUs
// without a workgroup) and walks K in 128-wide chunks; a wave owns 64 x 16 RT of it as 4 x RT
// v_mfma_f32_16x16x32_{bf16,f16} tiles, so a converted weight fragment feeds four MFMAs and an
// activation fragment RT of them (one ds_read_b128 per RT MFMAs: a quarter / half of what the LDS
// delivers per MFMA time).
//
//   * Activations: the chunk's [128][128] tile is staged through LDS, double-buffered: every thread
//     requests its eight 16-B pieces of chunk c + 1 before the MFMAs of chunk c and stores them after;
//     one barrier per chunk. Rows past M and columns past K are staged as zeros. Pieces are
//     XOR-swizzled by row (as in gemv_w8.hip); the k orders below read them conflict-free.
//   * Weights need no LDS: a lane loads the bytes of its own A fragments, row (lane & 15), and the K
//     order inside a chunk is permuted identically on the activation read addresses.
//       fp8:   16 B at k = 64 j + 16 g (g = lane >> 4, j = 0, 1): the first 8 bytes are the fragment
//              of step 2 j, the last 8 of step 2 j + 1 (activation piece 8 j + 2 g + h).
//       mxfp4, bf16: the 16 B of block g of the chunk with its scale byte; word s (elements 8 s .. 8 s + 7
//              of the block) is the fragment of step s (activation piece 4 g + s). The pieces of this
//              instantiation are swizzled by the row's bit pairs swapped -- under the plain row XOR two
//              lane groups of a ds_read_b128 would meet on the same banks. (With the fp16 order below
//              and four 4-byte loads per tile the bf16 kernel stopped at 380 TFLOP/s: docs/PERF.md,
//              Round 13.)
//       mxfp4, fp16: step s is block s of the chunk for every lane -- the word (8 nibbles) at byte
//              16 s + 4 g, elements 8 g .. 8 g + 7 of the block (activation piece 4 s + g) -- so an MFMA
//              never mixes blocks. Lane (row, g) loads the scale byte of (row, block g); a step fetches
//              the scales it needs from those lanes (ds_bpermute).
//   * mxfp4 block scales. bf16 has fp32's exponent range, so the scale rides in the conversion's scale
//     operand and the scaled element is exact. fp16 does not (6 * 2^14 overflows, 0.5 * 2^-30
//     flushes): there the conversion runs with scale 1, each step's MFMA goes into a zero accumulator
//     and the scales of the four weight rows a lane holds of the result (row 4 g + i in register i)
//     are applied in fp32, as in gemv_mx4.hip.
#include "common.h"

typedef unsigned int wq_u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 wq_f16x8 __attribute__((ext_vector_type(8)));

constexpr int WQ_KC = 128;  // K per chunk: 16 pieces of 8 activation elements per row (the swizzle's span)
constexpr int WQ_BM = 128;  // activation rows per workgroup
constexpr int WQ_MT = 4;    // 16-row activation tiles per wave (two waves along M)
constexpr int WQ_XP = WQ_BM * (WQ_KC / 8) / 256;  // 16-B activation pieces per thread per chunk

template <int DT, bool HI>
__device__ __forceinline__ uint32_t wq_cvt2_fp8(uint32_t w) {
  if constexpr (DT == 0) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
}
template <int DT, int SEL>
__device__ __forceinline__ uint32_t wq_cvt2_fp4(uint32_t w, float scale) {
  if constexpr (DT == 0) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, SEL));
}
// e8m0 byte -> 2^(E - 127) (E = 0: the fp32 subnormal 2^-127)
__device__ __forceinline__ float wq_e8m0(uint32_t e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }
__device__ __forceinline__ float wq_from_lane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}

template <int DT>
__device__ __forceinline__ f32x4 wq_mfma(const wq_u32x4& a, const wq_u32x4& b, const f32x4& c) {
  if constexpr (DT == 0)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(wq_f16x8, a), __builtin_bit_cast(wq_f16x8, b),
                                                  c, 0, 0, 0);
}

template <int DT>
__device__ __forceinline__ float wq_epilogue(float o, const uint16_t* bias, int n, int act) {
  if (bias) o += e2f<DT>(bias[n]);
  if (act == 1) o = gelu_tanh(o);
  else if (act == 2) o = 0.5f * o * (1.f + erff(o * 0.70710678118654752f));
  return o;
}

// a wave's weight registers for one chunk: fp8 two 16-B runs per tile, mxfp4 four words per tile (one
// block in bf16, a word of each block in fp16) and the scale of (row r16, block g)
template <int FMT, int RT>
struct WqW {
  wq_u32x4 w[RT][FMT == 0 ? 2 : 1];
  float e[RT];
};

template <int DT, int FMT, int RT>
__global__ __launch_bounds__(256, 2) void wq_gemm_kernel(const uint16_t* __restrict__ x, long long ldx,
                                                      const uint8_t* __restrict__ wq,
                                                      const void* __restrict__ wscale,
                                                      const uint16_t* __restrict__ bias,
                                                      uint16_t* __restrict__ y, long long ldy, int M, int N, int K,
                                                      int act, int vec) {
  constexpr int KC = WQ_KC, MT = WQ_MT, XP = WQ_XP;
  constexpr bool OWN = FMT == 1 && DT == 0;  // mxfp4 in bf16: a lane keeps one whole block of the chunk
  auto swz = [](int r) { return OWN ? ((r & 3) << 2) | ((r >> 2) & 3) : r & 15; };  // a row's piece swizzle
  constexpr int XS = WQ_BM * KC;  // one stage (elements)
  static_assert(2 * XS * 2 <= 65536, "static LDS");
  __shared__ __attribute__((aligned(16))) uint16_t xs[2 * XS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * WQ_BM;                               // the workgroup's first activation row
  const int mw = (wv & 1) * (MT * 16);                             // the wave's first row inside the tile
  const int n0 = blockIdx.x * (2 * RT * 16) + (wv >> 1) * (RT * 16);  // the wave's first weight row
  const int nc = (K + KC - 1) / KC;
  const int nb = K >> 5;  // mxfp4: blocks per row
  const long long wld = FMT == 0 ? K : (K >> 1);  // bytes per weight row
  const uint8_t* wrow[RT];
  const uint8_t* srow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {  // rows past N: a valid row, never stored
    const long long nr = min(n0 + rt * 16 + r16, N - 1);
    wrow[rt] = wq + nr * wld;
    srow[rt] = static_cast<const uint8_t*>(wscale) + nr * nb;
  }
  const int xp = tid & 15, xr0 = tid >> 4;  // this thread's piece column and first row of the stage

  auto load_w = [&](int c, WqW<FMT, RT>& W) {
    if constexpr (FMT == 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = c * KC + 64 * j + 16 * g;
          W.w[rt][j] = k < K ? *reinterpret_cast<const wq_u32x4*>(wrow[rt] + k) : wq_u32x4{0u, 0u, 0u, 0u};
        }
    } else {
      const int be = min(c * 4 + g, nb - 1);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if constexpr (OWN) {  // blocks past K: zero nibbles
          W.w[rt][0] = c * 4 + g < nb ? *reinterpret_cast<const wq_u32x4*>(wrow[rt] + c * (KC / 2) + 16 * g)
                                      : wq_u32x4{0u, 0u, 0u, 0u};
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            W.w[rt][0][s] =
                c * 4 + s < nb ? *reinterpret_cast<const uint32_t*>(wrow[rt] + c * (KC / 2) + 16 * s + 4 * g) : 0u;
        }
        W.e[rt] = wq_e8m0(srow[rt][be]);
      }
    }
  };
  auto load_x = [&](int c, wq_u32x4 (&xr)[XP]) {
    const int k = c * KC + xp * 8;
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int m = m0 + xr0 + 16 * i;
      xr[i] = (m < M && k < K) ? *reinterpret_cast<const wq_u32x4*>(x + (long long)m * ldx + k)
                               : wq_u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto store_x = [&](const wq_u32x4 (&xr)[XP], int buf) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int r = xr0 + 16 * i;
      *reinterpret_cast<wq_u32x4*>(xs + buf * XS + r * KC + ((xp ^ swz(r & 15)) << 3)) = xr[i];
    }
  };

  f32x4 acc[RT][MT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  wq_u32x4 XR[XP];
  // chunk c (workgroup-uniform): request c + 1, run the MFMAs of c from stage c & 1, stage c + 1
  auto step = [&](int c, const WqW<FMT, RT>& Wc, WqW<FMT, RT>& Wn) {
    if (c >= nc) return;
    if (c + 1 < nc) {
      load_w(c + 1, Wn);
      load_x(c + 1, XR);
    }
    const uint16_t* xb = xs + (c & 1) * XS + (mw + r16) * KC;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int piece = FMT == 0 ? 8 * (s >> 1) + 2 * g + (s & 1) : OWN ? 4 * g + s : 4 * s + g;
      wq_u32x4 bf[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        bf[mt] = *reinterpret_cast<const wq_u32x4*>(xb + mt * 16 * KC + ((piece ^ swz(r16)) << 3));
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if constexpr (FMT == 0) {
          const uint32_t w0 = Wc.w[rt][s >> 1][2 * (s & 1)], w1 = Wc.w[rt][s >> 1][2 * (s & 1) + 1];
          const wq_u32x4 af = {wq_cvt2_fp8<DT, false>(w0), wq_cvt2_fp8<DT, true>(w0), wq_cvt2_fp8<DT, false>(w1),
                               wq_cvt2_fp8<DT, true>(w1)};
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = wq_mfma<DT>(af, bf[mt], acc[rt][mt]);
        } else if constexpr (DT == 0) {
          const uint32_t wd = Wc.w[rt][0][s];
          const float sc = Wc.e[rt];  // (row r16, block g): this lane's own
          const wq_u32x4 af = {wq_cvt2_fp4<0, 0>(wd, sc), wq_cvt2_fp4<0, 1>(wd, sc), wq_cvt2_fp4<0, 2>(wd, sc),
                               wq_cvt2_fp4<0, 3>(wd, sc)};
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = wq_mfma<0>(af, bf[mt], acc[rt][mt]);
        } else {
          const uint32_t wd = Wc.w[rt][0][s];
          const wq_u32x4 af = {wq_cvt2_fp4<1, 0>(wd, 1.0f), wq_cvt2_fp4<1, 1>(wd, 1.0f), wq_cvt2_fp4<1, 2>(wd, 1.0f),
                               wq_cvt2_fp4<1, 3>(wd, 1.0f)};
          float sv[4];  // rows 4 g + i of block s: the C registers
#pragma unroll
          for (int i = 0; i < 4; ++i) sv[i] = wq_from_lane(Wc.e[rt], s * 16 + 4 * g + i);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 t = wq_mfma<1>(af, bf[mt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[rt][mt][i] = fmaf(sv[i], t[i], acc[rt][mt][i]);
          }
          // (pins the FMAs here: left alone the compiler sinks them below the staging stores, with every
          // step's zero-accumulator result live until then -- it spilled)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) asm volatile("" : "+v"(acc[rt][mt]));
        }
      }
    }
    if (c + 1 < nc) store_x(XR, (c + 1) & 1);
    __syncthreads();
  };
  WqW<FMT, RT> W0, W1;
  load_w(0, W0);
  load_x(0, XR);
  store_x(XR, 0);
  __syncthreads();
  for (int c = 0; c < nc; c += 2) {
    step(c, W0, W1);
    step(c + 1, W1, W0);
  }

  // a finished tile: weight rows n0 + 16 rt + 4 g + i (i < 4), activation row m0 + mw + 16 mt + r16
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int n = n0 + rt * 16 + 4 * g;
    if (n >= N) continue;
    float rs[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (FMT == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rs[i] = static_cast<const float*>(wscale)[min(n + i, N - 1)];
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + mw + mt * 16 + r16;
      if (m >= M) continue;
      uint32_t q[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float o = FMT == 0 ? rs[i] * acc[rt][mt][i] : acc[rt][mt][i];
        q[i] = n + i < N ? f2e<DT>(wq_epilogue<DT>(o, bias, n + i, act)) : 0u;
      }
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
}

// 128-row N tiles (RT = 4) once they give every one of the 256 CUs a workgroup; 64-row tiles otherwise
template <int DT, int FMT>
static void wq_go(const uint16_t* x, long long ldx, const uint8_t* wq, const void* wscale, const uint16_t* bias,
                  uint16_t* y, long long ldy, int M, int N, int K, int act, hipStream_t s) {
  const int vec = (ldy % 4 == 0 && ((uintptr_t)y & 7) == 0) ? 1 : 0;
  const unsigned mt = (unsigned)((M + WQ_BM - 1) / WQ_BM);
  const unsigned nt4 = (unsigned)((N + 127) / 128), nt2 = (unsigned)((N + 63) / 64);
  if ((long long)nt4 * mt >= 256)
    hipLaunchKernelGGL((wq_gemm_kernel<DT, FMT, 4>), dim3(nt4, mt), dim3(256), 0, s, x, ldx, wq, wscale, bias, y, ldy,
                       M, N, K, act, vec);
  else
    hipLaunchKernelGGL((wq_gemm_kernel<DT, FMT, 2>), dim3(nt2, mt), dim3(256), 0, s, x, ldx, wq, wscale, bias, y, ldy,
                       M, N, K, act, vec);
}

// x [M, K] 16-bit rows (row stride ldx elements). fmt 0: wq [N, K] e4m3 bytes, wscale [N] fp32; fmt 1:
// wq [N, K/2] e2m1 nibble pairs, wscale [N, K/32] e8m0 bytes (both contiguous). bias [N] of x's type
// (nullable), y [M, N] (row stride ldy). dt: 0 bf16, 1 fp16. Returns nonzero (nothing launched) for
// anything outside the kernel; the caller takes the reference path.
KCA_API int kca_wq_gemm(const void* x, long long ldx, const void* wq, const void* wscale, const void* bias, void* y,
                        long long ldy, int M, int N, int K, int act, int dt, int fmt, hipStream_t stream) {
  if (!x || !wq || !wscale || !y) return 1;
  if (fmt < 0 || fmt > 1 || dt < 0 || dt > 1 || act < 0 || act > 2) return 1;
  const int kq = fmt == 0 ? 16 : 32;
  if (M < 1 || N < 1 || K < kq || K % kq) return 1;
  if ((M + WQ_BM - 1) / WQ_BM > 65535) return 1;  // grid.y
  if (ldx < K || ldx % 8 || ldy < N) return 2;
  if (((uintptr_t)x & 15) || ((uintptr_t)wq & 15) || ((uintptr_t)y & 1) || ((uintptr_t)bias & 1)) return 2;
  if (fmt == 0 && ((uintptr_t)wscale & 3)) return 2;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint8_t* wp = static_cast<const uint8_t*>(wq);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  uint16_t* yp = static_cast<uint16_t*>(y);
  if (dt == 0 && fmt == 0) wq_go<0, 0>(xp, ldx, wp, wscale, bp, yp, ldy, M, N, K, act, stream);
  else if (dt == 0) wq_go<0, 1>(xp, ldx, wp, wscale, bp, yp, ldy, M, N, K, act, stream);
  else if (fmt == 0) wq_go<1, 0>(xp, ldx, wp, wscale, bp, yp, ldy, M, N, K, act, stream);
  else wq_go<1, 1>(xp, ldx, wp, wscale, bp, yp, ldy, M, N, K, act, stream);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}
