// Backward of the 3x3 / stride 1 / pad 1 NHWC bf16 convolution of conv_igemm.hip.
//
// Data gradient: gx = conv3x3(gy, wt) with wt[c, 2-r, 2-s, co] = w[co, r, s, c], so the forward kernel
// runs it unchanged (kca_conv3x3_fwd with C and Co swapped); this file only re-lays the weight:
//   * conv3x3_wflip_kernel: KRSC -> CRSK with the taps mirrored, one 64 x 64 (co, c) tile of one tap per
//     wave, 16-B pieces on both sides, the 8 x 8 blocks transposed in registers as transpose.hip does.
//
// Weight gradient: gw[co, tap, c] = sum_p gy[p, co] * x[shift_tap(p), c], p = (n, h, w); a shifted pixel
// in the padding contributes zero. GEMM view: M = Co, N = 9*C ordered (tap, channel), K = N*H*W pixels.
//   * conv3x3_wgrad_kernel: one workgroup = 128 co x 128 c of one tap over a range of 64-pixel chunks,
//     4 waves of 64 x 64 outputs (2 x 2 v_mfma_f32_32x32x16_bf16). Both operands are pixel-major in
//     memory while an MFMA operand wants the reduction index along a lane's registers, so the chunk's
//     [64 pixels][128 channels] row images of gy and of the tap-shifted x (padding rows written as
//     zeros, the forward's A predicate) are staged in LDS as 256-B rows with the XOR of toff() and
//     read back with ds_read_b64_tr_b16 (cdna_hip_programming.md T10, image (b)): two transposed reads
//     give a lane its 8 consecutive pixels of one channel. Register-staged (global -> VGPR ->
//     ds_write_b128), double-buffered, one barrier per chunk.
//   * The 9 taps of one (co tile, c tile, split) are adjacent workgroups on one XCD (xcd_remap): they
//     share the gy tile and re-read the same x pixels shifted.
//   * Split-K over the pixel chunks (uneven ranges allowed): split s writes fp32 partials
//     [S][Co][9][C] to the caller's workspace and conv3x3_wgrad_reduce_kernel sums them in split order
//     and writes bf16 -- no float atomics, two runs are bit-identical. With S = 1 the main kernel
//     writes bf16 directly.
// Tails: Co and C are multiples of 64, not of 128; rows / columns past the end stage zeros and are not
// stored.
#include "common.h"

namespace {

typedef unsigned int u32x4w __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------
// weight flip
__device__ __forceinline__ unsigned lo16(unsigned a, unsigned b) {  // (a.lo, b.lo)
  return __builtin_amdgcn_perm(b, a, 0x05040100u);
}
__device__ __forceinline__ unsigned hi16(unsigned a, unsigned b) {  // (a.hi, b.hi)
  return __builtin_amdgcn_perm(b, a, 0x07060302u);
}

// wt[c][8 - tap][co] = w[co][tap][c]; C, Co multiples of 64. blockIdx.y = tap, 4 tiles per workgroup.
__global__ void __launch_bounds__(256) conv3x3_wflip_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt,
                                                            int C, int Co) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tap = blockIdx.y;
  const int tiles_c = C >> 6;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= (Co >> 6) * tiles_c) return;
  const int tr = tile / tiles_c, tc = tile - tr * tiles_c;
  const int rb = lane & 7, cb = lane >> 3;
  const long long co0 = tr * 64 + rb * 8, c0 = tc * 64 + cb * 8;
  const bf16_t* in = w + (long long)tap * C;
  bf16_t* out = wt + (long long)(8 - tap) * Co;
  const long long ld_in = 9ll * C, ld_out = 9ll * Co;
  u32x4w a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = *reinterpret_cast<const u32x4w*>(in + (co0 + i) * ld_in + c0);
  // b[j] = channel c0 + j of the 8 output channels: word k holds rows (2k, 2k + 1)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    u32x4w bj;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned x = a[2 * k][j >> 1], y = a[2 * k + 1][j >> 1];
      bj[k] = (j & 1) ? hi16(x, y) : lo16(x, y);
    }
    *reinterpret_cast<u32x4w*>(out + (c0 + j) * ld_out + co0) = bj;
  }
}

// ---------------------------------------------------------------------------------------------------
// weight gradient
struct WgradArgs {
  const uint16_t* x;   // [N, H, W, C]
  const uint16_t* gy;  // [N, H, W, Co]
  uint16_t* gw;        // [Co, 3, 3, C]
  float* ws;           // [S, Co, 3, 3, C] (S > 1)
  int N, H, W, C, Co, S, nch;
};

constexpr int WBP = 64;             // pixels per K chunk
constexpr int WTILE = WBP * 256;    // bytes of one operand image: 64 rows of 128 channels
constexpr int WSTAGE = 2 * WTILE;   // gy image, then x image
constexpr unsigned kOOBW = 0x7ffffff0u;  // an offset past every buffer the kernel is given

// byte offset of 16-B chunk ch (0..15) of row `row` of a 256-B-row image (T10 image (b)): conflict-free
// for the transposed reads of the 32x32x16 operand; the store and the read go through the same map
__device__ __forceinline__ int toff(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef __attribute__((address_space(3))) char wlds_char;
typedef __attribute__((address_space(3))) s16x4 wlds_s16x4;

__device__ __forceinline__ bf16x8 tr_pair(wlds_char* lo, wlds_char* hi) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds_s16x4*)lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds_s16x4*)hi);
  const s16x8 c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}

__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_kernel(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nc = (a.C + 127) / 128;
  int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tap = t % 9;
  t /= 9;
  const int split = t % a.S;
  t /= a.S;
  const int c0 = (t % nc) * 128, co0 = (t / nc) * 128;
  const int dr = tap / 3 - 1, ds = tap % 3 - 1;
  const int k0 = (int)((long long)split * a.nch / a.S), k1 = (int)((long long)(split + 1) * a.nch / a.S);

  // load map: 16-B chunk ch of rows r0 + 16 i of both images
  const int ch = tid & 15, r0 = tid >> 4;
  const int gco = co0 + ch * 8, xc = c0 + ch * 8;
  const bool gok = gco < a.Co, xok = xc < a.C;
  const int HW = a.H * a.W;
  int ph[4], pw[4];  // (h, w) of this thread's 4 pixels of the next chunk to load
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rem = (k0 * WBP + r0 + 16 * i) % HW;  // (N*H*W*C*2 < 0x70000000: pixels fit an int)
    ph[i] = rem / a.W;
    pw[i] = rem - ph[i] * a.W;
  }
  const int dw = WBP % a.W, dh = (WBP / a.W) % a.H;  // one chunk further

  // buffer loads: a row in the padding or a channel past the end takes an offset past the buffer and
  // arrives as zeros (every real offset is below the 0x70000000 bound the entry point checks)
  const __amdgpu_buffer_rsrc_t bx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.x, (short)0, (int)((long long)a.N * HW * a.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t bg = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.gy, (short)0, (int)((long long)a.N * HW * a.Co * 2), 0x00020000);
  const int xshift = dr * a.W + ds;
  u32x4w rg[4], rx[4];
  auto load = [&](int k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = k * WBP + r0 + 16 * i;
      KCA_DASSERT(p < a.N * HW);
      const unsigned vg = gok ? (unsigned)(p * a.Co + gco) * 2u : kOOBW;
      const int hh = ph[i] + dr, ww = pw[i] + ds;
      const bool ok = xok && (unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W;
      const unsigned vx = ok ? (unsigned)((p + xshift) * a.C + xc) * 2u : kOOBW;
      rg[i] = __builtin_amdgcn_raw_buffer_load_b128(bg, vg, 0, 0);
      rx[i] = __builtin_amdgcn_raw_buffer_load_b128(bx, vx, 0, 0);
      pw[i] += dw;
      ph[i] += dh;
      if (pw[i] >= a.W) {
        pw[i] -= a.W;
        ++ph[i];
      }
      if (ph[i] >= a.H) ph[i] -= a.H;
    }
  };
  auto store = [&](int buf) {
    char* G = wsm + buf * WSTAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4w*>(G + toff(r0 + 16 * i, ch)) = rg[i];
      *reinterpret_cast<u32x4w*>(G + WTILE + toff(r0 + 16 * i, ch)) = rx[i];
    }
  };

  // transposed-read addresses (bytes from the stage base) of k-step 0; k-step ks adds 16 rows = 4096 B
  // (the XOR term of toff() depends on row & 15 only). Lane 4q + p of a 16-lane group supplies row q,
  // elements 4p .. 4p + 3 of its group's 4 x 16 block and receives the block's column (lane & 15):
  // groups 0 / 1 take channels 0-15 / 16-31 of pixels 0-7 of the k-step, groups 2 / 3 those of pixels
  // 8-15; read t takes pixels 4t .. 4t + 3 of the lane's 8.
  const int g1 = (lane >> 4) & 1, hf = lane >> 5, q = (lane & 15) >> 2, pp = lane & 3;
  int fa[2][2], fb[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int row = 8 * hf + 4 * tt + q;
      fa[i][tt] = toff(row, 8 * wm + 4 * i + 2 * g1 + (pp >> 1)) + 8 * (pp & 1);
      fb[i][tt] = WTILE + toff(row, 8 * wn + 4 * i + 2 * g1 + (pp >> 1)) + 8 * (pp & 1);
    }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // a wave whose 64 x 64 outputs lie wholly past Co or C (320 = 2.5 tiles) stages its share of the
  // images and leaves the matrix core to the workgroup it shares the CU with (wave-uniform: the
  // transposed reads of the live waves run with EXEC all ones)
  const bool live = co0 + wm * 64 < a.Co && c0 + wn * 64 < a.C;
  wlds_char* lsm = (wlds_char*)wsm;
  load(k0);
  store(0);
  __syncthreads();
  for (int k = k0; k < k1; ++k) {
    const int buf = (k - k0) & 1;
    if (k + 1 < k1) load(k + 1);
    wlds_char* S = lsm + buf * WSTAGE;
    if (live) {
      // fragments of k-step ks + 1 requested before the MFMAs of ks (pinned, as in the forward)
      bf16x8 af[2][2], bf[2][2];
      auto rd = [&](int ks, int sl) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          af[sl][i] = tr_pair(S + fa[i][0] + 4096 * ks, S + fa[i][1] + 4096 * ks);
          bf[sl][i] = tr_pair(S + fb[i][0] + 4096 * ks, S + fb[i][1] + 4096 * ks);
        }
      };
      rd(0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
      for (int ks = 0; ks < WBP / 16; ++ks) {
        if (ks + 1 < WBP / 16) {
          rd(ks + 1, (ks + 1) & 1);
          __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks & 1][i], bf[ks & 1][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
      }
    }
    if (k + 1 < k1) store(buf ^ 1);
    __syncthreads();
  }

  // accumulator (i, j): column lane & 31 is the channel, rows the output channels
  const int col = lane & 31;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + wn * 64 + j * 32 + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * hf + (r & 3);
        if (co < a.Co && c < a.C) {
          const long long o = ((long long)co * 9 + tap) * a.C + c;
          if (a.S == 1) a.gw[o] = f2bf(acc[i][j][r]);
          else a.ws[(long long)split * a.Co * 9 * a.C + o] = acc[i][j][r];
        }
      }
    }
}

// gw = bf16(sum_s ws[s]) in split order, 4 elements per thread
__global__ void __launch_bounds__(256) conv3x3_wgrad_reduce_kernel(const float* __restrict__ ws,
                                                                   bf16_t* __restrict__ gw, long long total, int S) {
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += stride) {
    f32x4 s = *reinterpret_cast<const f32x4*>(ws + i);
    for (int k = 1; k < S; ++k) s += *reinterpret_cast<const f32x4*>(ws + k * total + i);
    U16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o.v[e] = f2bf(s[e]);
    *reinterpret_cast<U16x4*>(gw + i) = o;
  }
}

constexpr long long kMaxBytes = 0x70000000ll;  // the forward's buffer bound

bool wgrad_shape_ok(int N, int H, int W, int C, int Co) {
  if (N < 1 || H < 1 || W < 1 || C < 64 || Co < 64 || C % 64 || Co % 64) return false;
  const long long npix = (long long)N * H * W;
  return npix % 128 == 0 && npix * C * 2 < kMaxBytes && npix * Co * 2 < kMaxBytes &&
         (long long)Co * 9 * C * 2 < kMaxBytes;
}

long long wgrad_tiles(int C, int Co) { return (long long)((Co + 127) / 128) * ((C + 127) / 128) * 9; }

}  // namespace

// wt [C, 3, 3, Co] = w [Co, 3, 3, C] transposed with the taps mirrored (the data gradient's weight)
KCA_API int kca_conv3x3_wflip(const void* w, void* wt, int C, int Co, hipStream_t stream) {
  if (C < 64 || Co < 64 || C % 64 || Co % 64 || (long long)Co * 9 * C * 2 >= kMaxBytes) return 1;
  if (((uintptr_t)w | (uintptr_t)wt) & 15) return 2;
  const int tiles = (Co / 64) * (C / 64);
  hipLaunchKernelGGL(conv3x3_wflip_kernel, dim3((unsigned)((tiles + 3) / 4), 9), dim3(256), 0, stream,
                     (const bf16_t*)w, (bf16_t*)wt, C, Co);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}

// automatic split count: the workgroups (two per CU fit: 64 KB LDS each) fill the 256 CUs' 512 slots
// once without a tail round; 0 for unsupported shapes
KCA_API int kca_conv3x3_wgrad_splits(int N, int H, int W, int C, int Co) {
  if (!wgrad_shape_ok(N, H, W, C, Co)) return 0;
  const long long nch = (long long)N * H * W / WBP, tiles = wgrad_tiles(C, Co);
  long long s = 512 / tiles;
  if (s > nch) s = nch;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

// gw [Co, 3, 3, C] = weight gradient of conv3x3 from x [N, H, W, C] and gy [N, H, W, Co] (bf16). splits
// 0: automatic; S > 1 needs ws of S * Co * 9 * C floats. Returns 1 (nothing launched) for unsupported
// shapes, 2 for misaligned / missing buffers.
KCA_API int kca_conv3x3_wgrad(const void* x, const void* gy, void* gw, void* ws, int N, int H, int W, int C, int Co,
                              int splits, hipStream_t stream) {
  if (!wgrad_shape_ok(N, H, W, C, Co) || splits < 0) return 1;
  const int nch = (int)((long long)N * H * W / WBP);
  int S = splits ? splits : kca_conv3x3_wgrad_splits(N, H, W, C, Co);
  if (S > nch) S = nch;
  const long long tiles = wgrad_tiles(C, Co), total = (long long)Co * 9 * C;
  if (tiles * S > (1ll << 30) || total * 4 * S >= (1ll << 40)) return 1;
  if (((uintptr_t)x | (uintptr_t)gy | (uintptr_t)gw) & 15) return 2;
  if (S > 1 && (!ws || ((uintptr_t)ws & 15))) return 2;
  const WgradArgs a{(const uint16_t*)x, (const uint16_t*)gy, (uint16_t*)gw, (float*)ws, N, H, W, C, Co, S, nch};
  hipLaunchKernelGGL(conv3x3_wgrad_kernel, dim3((unsigned)(tiles * S)), dim3(256), 2 * WSTAGE, stream, a);
  if (hipGetLastError() != hipSuccess) return 4;
  if (S > 1) {
    hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3(kca_grid(total / 4, 256)), dim3(256), 0, stream,
                       (const float*)ws, (bf16_t*)gw, total, S);
    if (hipGetLastError() != hipSuccess) return 4;
  }
  return 0;
}
