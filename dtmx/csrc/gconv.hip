// Grouped 3x3 convolution (fwd / dgrad / wgrad) for gfx950, NHWC.
// (reference src/operator/nn/convolution.cu with num_group > 1 — the
// cardinality-32 3x3 of every ResNeXt block.)
//
// C_in == C_out == C, Cg = C / groups in {4, 8, 16, 32}. A 32-channel tile of
// such a conv is a dense 32 -> 32 3x3 conv whose per-tap weight is block
// diagonal (32/Cg blocks of Cg x Cg), so every width runs the same MFMA
// tile: v_mfma_f32_16x16x32 with the zero-expanded weight as the A operand
// and 16 pixels x 32 channels of the activation as the B operand.
//
//   fwd / dgrad  D[32 ch out][16 px] += Wtap[32 out][32 in] . X[32 in][16 px]
//                The B fragment of lane l is 8 consecutive channels of pixel
//                l & 15 — one 16-byte NHWC load, no LDS. The weight rows are
//                permuted when packed so that a lane's 2 x 4 accumulators are
//                8 consecutive output channels: one 16-byte store.
//   wgrad        D[co][ci] += dY[co][32 px] . X[32 px][ci] contracts over
//                pixels; both operands are read pixel-major out of a wave
//                private LDS image with ds_read_b64_tr_b16. Only the diagonal
//                16x16 blocks are computed for Cg <= 16.
//
// The packed weight (fragment order, zero-expanded) is made per call by a
// small kernel on the current stream; nothing is cached.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"

namespace dtmx {

static hipStream_t gc_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int GC_THREADS = 256;    // 4 waves
constexpr int GC_WAVES = GC_THREADS / 64;
constexpr int GC_CT = 32;          // channels per tile
constexpr int GC_MT = 4;           // fwd/dgrad: 16-pixel MFMA tiles per wave step
constexpr int GC_BLOCKS = 1024;    // fwd/dgrad/wgrad: target grid size
constexpr int GC_WG_KT = 32;       // wgrad: pixels per contraction step
constexpr int GC_WG_MIN_STEPS = 4; // wgrad: steps per wave before splitting further
constexpr long GC_WG_WS_BYTES = 32l << 20;  // wgrad: workspace cap
constexpr int GC_FIN_I = 16;       // finalize: outputs per block ...
constexpr int GC_FIN_B = 16;       // ... x partial slices per output
constexpr int GC_WG_IMG = GC_WG_KT * GC_CT * 2;  // one [32 px][32 ch] image, bytes

static_assert(GC_FIN_I * GC_FIN_B == GC_THREADS, "finalize block shape");
static_assert(GC_WAVES * 4 * GC_WG_IMG >= GC_WAVES * 4 * 64 * 16,
              "wgrad: the block reduce reuses the image LDS");

template <typename elem_t>
__device__ __forceinline__ typename E8<elem_t>::v8 gc_zero() {
  typename E8<elem_t>::v8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (elem_t)0.f;
  return z;
}

// ------------------------------------------------------------- weight pack

// wp[ct][tap][nh][lane] (8 elements each) is the A fragment of MFMA `nh` of
// tap `tap` of channel tile `ct`: A[row i = lane & 15][k = 8 (lane >> 4) + j].
// Row i of MFMA nh is output-side channel 8 (i >> 2) + 4 nh + (i & 3) of the
// tile, so accumulator register r of lane group g is channel 8 g + 4 nh + r.
// fwd: output side = co, contraction = ci. dgrad (TRANSPOSE): output side =
// ci, contraction = co; the tap keeps its forward index. Elements outside the
// diagonal Cg x Cg blocks are zero. The weight is read through its strides,
// so both dense layouts of (C, Cg, 3, 3) pack the same way.
template <typename elem_t>
__global__ __launch_bounds__(GC_THREADS) void gconv_pack_kernel(
    const elem_t* __restrict__ w, elem_t* __restrict__ wp, uint32_t total,
    uint32_t Cg, long s0, long s1, long s2, long s3, bool transpose) {
  using V8 = typename E8<elem_t>::v8;
  uint32_t i = blockIdx.x * GC_THREADS + threadIdx.x;
  if (i >= total) return;
  uint32_t lane = i & 63, nh = (i >> 6) & 1, r = i >> 7;
  uint32_t ct = r / 9, tap = r - ct * 9;
  uint32_t row = lane & 15, g = lane >> 4;
  uint32_t oc = 8 * (row >> 2) + 4 * nh + (row & 3);
  uint32_t kh = tap / 3, kw = tap - kh * 3;
  V8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t kc = 8 * g + j;
    uint32_t co = transpose ? kc : oc, ci = transpose ? oc : kc;
    elem_t e = (elem_t)0.f;
    if (co / Cg == ci / Cg)
      e = w[(long)(ct * GC_CT + co) * s0 + (long)(ci % Cg) * s1 + kh * s2 + kw * s3];
    v[j] = e;
  }
  ((V8*)wp)[i] = v;
}

// ---------------------------------------------------------- forward, dgrad

// One axis of one tap. The written tensor is walked as a sub-grid: written
// coordinate = o * OS + A (A = parity class, dgrad stride 2 only); the tap
// reads coordinate o * IS + OFF of the other tensor and is `on` only where
// that is an integer: for dgrad h + PAD - k must be divisible by the stride.
template <int STRIDE, int PAD, bool DGRAD, int A, int K>
struct GcTap {
  static constexpr bool on = DGRAD ? ((A + PAD - K) % STRIDE == 0) : true;
  static constexpr int IS = DGRAD ? 1 : STRIDE;
  static constexpr int OFF = DGRAD ? (A + PAD - K) / STRIDE : K - PAD;
};

// All pixels of one parity class (A, B) of the written tensor `dst`
// (N, DH, DW, C); fwd and stride-1 dgrad have the single class (0, 0).
// SUBH x SUBW is the class's sub-grid. A wave owns channel tile `ct` and
// walks steps of GC_MT x 16 pixels, blockIdx.x apart.
template <typename elem_t, int STRIDE, int PAD, bool DGRAD, int A, int B>
__device__ __forceinline__ void gc_class(
    const elem_t* __restrict__ src, elem_t* __restrict__ dst,
    const typename E8<elem_t>::v8 (&wf)[9][2], uint32_t N, uint32_t C,
    uint32_t SH, uint32_t SW, uint32_t DH, uint32_t DW_, uint32_t SUBH,
    uint32_t SUBW, FastDiv dSubH, FastDiv dSubW, uint32_t ct, uint32_t lane) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int OS = DGRAD ? STRIDE : 1;
  const uint32_t total = N * SUBH * SUBW;
  const uint32_t nsteps = (total + 16 * GC_MT - 1) / (16 * GC_MT);
  const uint32_t r = lane & 15, g = lane >> 4;
  const uint32_t coff = ct * GC_CT + 8 * g;
  for (uint32_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
    f32x4 acc[GC_MT][2];
    int oh[GC_MT], ow[GC_MT];
    uint32_t nn[GC_MT];
    bool live[GC_MT];
#pragma unroll
    for (int s = 0; s < GC_MT; ++s) {
      uint32_t m = (step * GC_MT + s) * 16 + r;
      live[s] = m < total;
      m = live[s] ? m : 0;
      uint32_t t = dSubW.div(m);
      ow[s] = (int)dSubW.mod(m, t);
      nn[s] = dSubH.div(t);
      oh[s] = (int)dSubH.mod(t, nn[s]);
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[s][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      // the three GcTap<..., kh> of this unrolled iteration
      const bool hon = kh == 0 ? GcTap<STRIDE, PAD, DGRAD, A, 0>::on
                     : kh == 1 ? GcTap<STRIDE, PAD, DGRAD, A, 1>::on
                               : GcTap<STRIDE, PAD, DGRAD, A, 2>::on;
      const int hoff = kh == 0 ? GcTap<STRIDE, PAD, DGRAD, A, 0>::OFF
                     : kh == 1 ? GcTap<STRIDE, PAD, DGRAD, A, 1>::OFF
                               : GcTap<STRIDE, PAD, DGRAD, A, 2>::OFF;
      if (!hon) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const bool won = kw == 0 ? GcTap<STRIDE, PAD, DGRAD, B, 0>::on
                       : kw == 1 ? GcTap<STRIDE, PAD, DGRAD, B, 1>::on
                                 : GcTap<STRIDE, PAD, DGRAD, B, 2>::on;
        const int woff = kw == 0 ? GcTap<STRIDE, PAD, DGRAD, B, 0>::OFF
                       : kw == 1 ? GcTap<STRIDE, PAD, DGRAD, B, 1>::OFF
                                 : GcTap<STRIDE, PAD, DGRAD, B, 2>::OFF;
        if (!won) continue;
        constexpr int IS = GcTap<STRIDE, PAD, DGRAD, 0, 0>::IS;
        V8 xv[GC_MT];
#pragma unroll
        for (int s = 0; s < GC_MT; ++s) {
          int ih = oh[s] * IS + hoff, iw = ow[s] * IS + woff;
          bool ok = live[s] && (uint32_t)ih < SH && (uint32_t)iw < SW;
          xv[s] = ok ? *(const V8*)(src + (((size_t)nn[s] * SH + (uint32_t)ih) * SW +
                                           (uint32_t)iw) * C + coff)
                     : gc_zero<elem_t>();
        }
#pragma unroll
        for (int s = 0; s < GC_MT; ++s)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            acc[s][h] = E8<elem_t>::mfma(wf[kh * 3 + kw][h], xv[s], acc[s][h]);
      }
    }
    // lane (r, g) holds channels 8g .. 8g+7 of its pixel: one 16-byte store
#pragma unroll
    for (int s = 0; s < GC_MT; ++s) {
      if (!live[s]) continue;
      V8 o;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * h + e] = (elem_t)acc[s][h][e];
      *(V8*)(dst + (((size_t)nn[s] * DH + (uint32_t)(oh[s] * OS + A)) * DW_ +
                    (uint32_t)(ow[s] * OS + B)) * C + coff) = o;
    }
  }
}

// src is read, dst is written: fwd (x -> y) or dgrad (dy -> dx). grid =
// (pixel steps, ceil(CT / 4)); the four waves of a block take four adjacent
// channel tiles of the same pixels (256 contiguous bytes per pixel) and keep
// their 9 x 2 weight fragments in registers across steps. Borders are
// predicated loads of zero; every dst element of the tile is written.
// Stride-2 dgrad walks the four (h, w) parity classes in turn: within a
// class the contributing taps are a compile-time set (4 + 2 + 2 + 1 = 9).
template <typename elem_t, int STRIDE, int PAD, bool DGRAD>
__global__ __launch_bounds__(GC_THREADS) void gconv_gather_kernel(
    const elem_t* __restrict__ src, const elem_t* __restrict__ wp,
    elem_t* __restrict__ dst, uint32_t N, uint32_t C, uint32_t SH, uint32_t SW,
    uint32_t DH, uint32_t DW_, FastDiv dH0, FastDiv dW0, FastDiv dH1,
    FastDiv dW1) {
  using V8 = typename E8<elem_t>::v8;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t ct = blockIdx.y * GC_WAVES + (threadIdx.x >> 6);
  if (ct * GC_CT >= C) return;  // whole wave; no block barrier below
  V8 wf[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      wf[t][h] = ((const V8*)wp)[((ct * 9 + t) * 2 + h) * 64 + lane];
  if constexpr (DGRAD && STRIDE == 2) {
    gc_class<elem_t, 2, PAD, true, 0, 0>(src, dst, wf, N, C, SH, SW, DH, DW_, dH0.d,
                                         dW0.d, dH0, dW0, ct, lane);
    if (dW1.d > 0 && DW_ > 1)
      gc_class<elem_t, 2, PAD, true, 0, 1>(src, dst, wf, N, C, SH, SW, DH, DW_, dH0.d,
                                           dW1.d, dH0, dW1, ct, lane);
    if (dH1.d > 0 && DH > 1) {
      gc_class<elem_t, 2, PAD, true, 1, 0>(src, dst, wf, N, C, SH, SW, DH, DW_, dH1.d,
                                           dW0.d, dH1, dW0, ct, lane);
      if (dW1.d > 0 && DW_ > 1)
        gc_class<elem_t, 2, PAD, true, 1, 1>(src, dst, wf, N, C, SH, SW, DH, DW_,
                                             dH1.d, dW1.d, dH1, dW1, ct, lane);
    }
  } else {
    gc_class<elem_t, STRIDE, PAD, DGRAD, 0, 0>(src, dst, wf, N, C, SH, SW, DH, DW_,
                                               dH0.d, dW0.d, dH0, dW0, ct, lane);
  }
}

// -------------------------------------------------------------------- wgrad

// One MFMA operand out of a [32 px][32 ch] LDS image (64-byte rows): lane l
// gets channel 16 half + (l & 15), pixels 8 (l >> 4) .. + 7. Two transposed
// reads of a [4 px][16 ch] block each (cdna_hip_programming.md T10): lane
// 4q + p of a 16-lane group supplies row q, channels 4p .. 4p+3.
template <typename elem_t>
__device__ __forceinline__ void gc_tr_frags(const char* img, uint32_t lane,
                                            typename E8<elem_t>::v8 (&f)[2]) {
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_;
  union Frag {
    typename E8<elem_t>::v8 v;
    u32x2_ h[2];
  };
  const uint32_t i = lane & 15, g = lane >> 4;
  const unsigned a0 =
      (unsigned)(uintptr_t)img + (8 * g + (i >> 2)) * 64 + (i & 3) * 8;
  const unsigned a1 = a0 + 4 * 64, a2 = a0 + 32, a3 = a1 + 32;
  u32x2_ t0, t1, t2, t3;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);  // keep the MFMAs below the asm's wait
  Frag fr;
  fr.h[0] = t0; fr.h[1] = t1; f[0] = fr.v;
  fr.h[0] = t2; fr.h[1] = t3; f[1] = fr.v;
}

// Stage 1. grid = (NB pixel slices, channel tiles). Each wave walks
// 32-pixel contraction steps NB * 4 apart: it gathers dy and, per tap, the
// shifted x pixels (zero outside the image) into its private LDS images with
// 16-byte loads, reads both operands back pixel-major and accumulates
// D[co][ci] per tap in registers — the two diagonal 16x16 blocks for
// Cg <= 16, all four for Cg == 32 (FULL). The block then adds its four waves
// in wave order through LDS and writes part[blockIdx.x][9][C][Cg]: only the
// diagonal Cg x Cg blocks, every element of its own channel tile.
template <typename elem_t, int STRIDE, bool FULL>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_partial_kernel(
    const elem_t* __restrict__ x, const elem_t* __restrict__ dy,
    float* __restrict__ part, uint32_t C, uint32_t Cg, uint32_t H, uint32_t W,
    uint32_t M, uint32_t ksteps, int pad, FastDiv dQ, FastDiv dP) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int NBLK = FULL ? 4 : 2;
  __shared__ __attribute__((aligned(16))) char smem[GC_WAVES * 4 * GC_WG_IMG];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t ct = blockIdx.y;
  char* img = smem + wv * 4 * GC_WG_IMG;  // [0] dy, [1..3] x of taps kw = 0..2
  f32x4 acc[9][NBLK];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int b = 0; b < NBLK; ++b) acc[t][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging slot s = lane + 64 i holds pixel s >> 2, 8-channel chunk s & 3
  const uint32_t coff = ct * GC_CT + (lane & 3) * 8;
  for (uint32_t ks = blockIdx.x * GC_WAVES + wv; ks < ksteps;
       ks += gridDim.x * GC_WAVES) {
    int ih0[2], iw0[2];
    uint32_t nn[2];
    bool live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint32_t m = ks * GC_WG_KT + (lane >> 2) + 16 * i;
      live[i] = m < M;
      V8 v = live[i] ? *(const V8*)(dy + (size_t)m * C + coff) : gc_zero<elem_t>();
      *(V8*)(img + (lane + 64 * i) * 16) = v;
      m = live[i] ? m : 0;
      uint32_t t = dQ.div(m), q = dQ.mod(m, t);
      nn[i] = dP.div(t);
      uint32_t p = dP.mod(t, nn[i]);
      ih0[i] = (int)(p * STRIDE) - pad;
      iw0[i] = (int)(q * STRIDE) - pad;
    }
    V8 gy[2];
    gc_tr_frags<elem_t>(img, lane, gy);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          int ih = ih0[i] + kh, iw = iw0[i] + kw;
          bool ok = live[i] && (uint32_t)ih < H && (uint32_t)iw < W;
          V8 v = ok ? *(const V8*)(x + (((size_t)nn[i] * H + (uint32_t)ih) * W +
                                        (uint32_t)iw) * C + coff)
                    : gc_zero<elem_t>();
          *(V8*)(img + (1 + kw) * GC_WG_IMG + (lane + 64 * i) * 16) = v;
        }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        V8 xf[2];
        gc_tr_frags<elem_t>(img + (1 + kw) * GC_WG_IMG, lane, xf);
        const int t = kh * 3 + kw;
        if (FULL) {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[t][b] = E8<elem_t>::mfma(gy[b >> 1], xf[b & 1], acc[t][b]);
        } else {
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[t][b] = E8<elem_t>::mfma(gy[b], xf[b], acc[t][b]);
        }
      }
    }
  }
  // fixed-order fold over the block's waves, one tap at a time
  f32x4* red = (f32x4*)smem;  // [wave][NBLK][64 lanes]
  const uint32_t b = wv;      // the 16x16 block this thread folds and writes
  const uint32_t hc = FULL ? b >> 1 : b, hi = FULL ? b & 1 : b;
  const uint32_t ci = hi * 16 + (lane & 15);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NBLK; ++k) red[(wv * NBLK + k) * 64 + lane] = acc[t][k];
    __syncthreads();
    if (b < (uint32_t)NBLK) {
      f32x4 s = red[b * 64 + lane];
#pragma unroll
      for (int w_ = 1; w_ < GC_WAVES; ++w_) {
        f32x4 o = red[(w_ * NBLK + b) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += o[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t co = hc * 16 + (lane >> 4) * 4 + e;
        if (co / Cg == ci / Cg)
          part[(((size_t)blockIdx.x * 9 + t) * C + ct * GC_CT + co) * Cg + ci % Cg] =
              s[e];
      }
    }
  }
}

// Stage 2. Sums part[0..NB) for each of the 9*C*Cg outputs in a fixed order,
// converts and writes dw in the parameter's layout: [C][Cg][3][3], or
// [C][3][3][Cg] when w_cl. A block is GC_FIN_I outputs x GC_FIN_B slices.
template <typename elem_t>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_finalize_kernel(
    const float* __restrict__ part, elem_t* __restrict__ dw, uint32_t C,
    uint32_t Cg, uint32_t NB, bool w_cl) {
  __shared__ float red[GC_FIN_B][GC_FIN_I];
  const uint32_t il = threadIdx.x % GC_FIN_I, b = threadIdx.x / GC_FIN_I;
  const uint32_t i = blockIdx.x * GC_FIN_I + il;  // index into [9][C][Cg]
  const uint32_t ccg = C * Cg, n = 9 * ccg;
  float s = 0.f;
  if (i < n)
    for (uint32_t k = b; k < NB; k += GC_FIN_B) s += part[(size_t)k * n + i];
  red[b][il] = s;
  __syncthreads();
  if (b == 0 && i < n) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < GC_FIN_B; ++k) tot += red[k][il];
    uint32_t t = i / ccg, r = i - t * ccg;
    uint32_t co = r / Cg, cg = r - co * Cg;
    size_t o = w_cl ? ((size_t)co * 9 + t) * Cg + cg : ((size_t)co * Cg + cg) * 9 + t;
    dw[o] = (elem_t)tot;
  }
}

// --------------------------------------------------------------- host side

static bool gc_is_16(const at::Tensor& t) {
  return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf;
}

// logical NCHW with channels_last strides; size-1 dims may carry any stride
static bool gc_is_nhwc(const at::Tensor& t) {
  if (t.dim() != 4) return false;
  long C = t.size(1), H = t.size(2), W = t.size(3);
  long want[4] = {H * W * C, 1, W * C, C};
  for (int d = 0; d < 4; ++d)
    if (t.size(d) > 1 && t.stride(d) != want[d]) return false;
  return true;
}

static bool gc_aligned16(const at::Tensor& t) {
  return ((uintptr_t)t.data_ptr() & 15) == 0;
}

static void gc_check_act(const char* op, const char* name, const at::Tensor& a) {
  TORCH_CHECK(a.is_cuda() && gc_is_16(a), op, ": ", name,
              " must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(a.dim() == 4 && a.numel() > 0, op, ": ", name,
              " must be a non-empty 4-D (N,C,H,W) tensor");
  TORCH_CHECK(gc_is_nhwc(a), op, ": ", name,
              " must be channels_last (NHWC) in memory");
  TORCH_CHECK(gc_aligned16(a), op, ": ", name, " must be 16-byte aligned");
  TORCH_CHECK(a.numel() < (1ll << 31), op, ": ", name, " too large (>= 2^31 elements)");
}

static void gc_check_sp(const char* op, long stride, long pad) {
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ", stride);
  TORCH_CHECK(pad == 0 || pad == 1, op, ": padding must be 0 or 1, got ", pad);
}

// C, groups -> Cg
static long gc_check_groups(const char* op, long C, long groups) {
  TORCH_CHECK(groups > 1 && C % groups == 0, op,
              ": groups must be > 1 and divide C, got C=", C, " groups=", groups);
  long Cg = C / groups;
  TORCH_CHECK(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32, op,
              ": grouped kernels need channels per group in {4, 8, 16, 32}, got ", Cg);
  TORCH_CHECK(C % 32 == 0, op, ": grouped kernels need C % 32 == 0, got C=", C);
  return Cg;
}

// returns true when the weight's memory is channels_last, [C][3][3][Cg]
static bool gc_check_w(const char* op, const at::Tensor& w, const at::Tensor& a,
                       long Cg) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == a.scalar_type() &&
                  w.device() == a.device(),
              op, ": weight must be on the same device and of the same dtype");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3, op,
              ": grouped kernels support 3x3 weights only");
  TORCH_CHECK(w.size(0) == a.size(1), op,
              ": grouped kernels need in_channels == out_channels; weight has ",
              w.size(0), " output channels, the activation has ", a.size(1));
  TORCH_CHECK(w.size(1) == Cg, op, ": weight has ", w.size(1),
              " channels per group, C / groups is ", Cg);
  bool contig = w.stride(0) == 9 * Cg && w.stride(1) == 9 && w.stride(2) == 3 &&
                w.stride(3) == 1;
  bool cl = w.stride(0) == 9 * Cg && w.stride(1) == 1 && w.stride(2) == 3 * Cg &&
            w.stride(3) == Cg;
  TORCH_CHECK(contig || cl, op,
              ": weight memory must be dense [C][Cg][3][3] or [C][3][3][Cg]");
  TORCH_CHECK(gc_aligned16(w), op, ": weight must be 16-byte aligned");
  return cl;
}

static bool gc_out_dims(long H, long W, long stride, long pad, long& P, long& Q) {
  if (H + 2 * pad < 3 || W + 2 * pad < 3) return false;
  P = (H + 2 * pad - 3) / stride + 1;
  Q = (W + 2 * pad - 3) / stride + 1;
  return true;
}

static at::Tensor gc_pack(const at::Tensor& w, long C, long Cg, bool transpose) {
  auto wp = at::empty({C / GC_CT, 9, 2, 64, 8}, w.options());
  uint32_t total = (uint32_t)(C / GC_CT) * 9 * 2 * 64;
  DTMX_DISPATCH_16(w.scalar_type(), "gconv_pack", {
    gconv_pack_kernel<elem_t>
        <<<(total + GC_THREADS - 1) / GC_THREADS, GC_THREADS, 0, gc_stream()>>>(
            (const elem_t*)w.data_ptr(), (elem_t*)wp.data_ptr(), total, (uint32_t)Cg,
            w.stride(0), w.stride(1), w.stride(2), w.stride(3), transpose);
  });
  return wp;
}

// grid for the gather kernel: x = pixel steps (grid-strided past the cap so a
// wave reuses its weight fragments), y = groups of four channel tiles
static dim3 gc_gather_grid(long pixels, long C) {
  uint32_t gy = (uint32_t)((C / GC_CT + GC_WAVES - 1) / GC_WAVES);
  uint32_t steps = (uint32_t)((pixels + 16 * GC_MT - 1) / (16 * GC_MT));
  uint32_t cap = GC_BLOCKS / gy;
  if (cap < 1) cap = 1;
  uint32_t gx = steps < cap ? steps : cap;
  return dim3(gx < 1 ? 1 : gx, gy);
}

at::Tensor gconv_fwd(const at::Tensor& x, const at::Tensor& w, long stride, long pad,
                     long groups) {
  const char* op = "gconv_fwd";
  gc_check_act(op, "x", x);
  gc_check_sp(op, stride, pad);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == x.size(1), op,
              ": grouped kernels need in_channels == out_channels; weight has ",
              w.dim() == 4 ? w.size(0) : -1, " output channels, x has ", x.size(1));
  long N = x.size(0), C = x.size(1), H = x.size(2), W_ = x.size(3), P, Q;
  long Cg = gc_check_groups(op, C, groups);
  gc_check_w(op, w, x, Cg);
  TORCH_CHECK(gc_out_dims(H, W_, stride, pad, P, Q),
              "gconv_fwd: input smaller than the 3x3 window");
  auto y = at::empty({N, C, P, Q}, x.options(), at::MemoryFormat::ChannelsLast);
  auto wp = gc_pack(w, C, Cg, false);
  FastDiv dH, dW, none;
  dH.init((uint32_t)P);
  dW.init((uint32_t)Q);
  none.init(1);
  dim3 grid = gc_gather_grid(N * P * Q, C);
#define DTMX_GC_FWD(S_, P_)                                                        \
  gconv_gather_kernel<elem_t, S_, P_, false><<<grid, GC_THREADS, 0, gc_stream()>>>( \
      (const elem_t*)x.data_ptr(), (const elem_t*)wp.data_ptr(),                   \
      (elem_t*)y.data_ptr(), N, C, H, W_, P, Q, dH, dW, none, none)
  DTMX_DISPATCH_16(x.scalar_type(), "gconv_fwd", {
    if (stride == 1 && pad == 0) DTMX_GC_FWD(1, 0);
    else if (stride == 1) DTMX_GC_FWD(1, 1);
    else if (pad == 0) DTMX_GC_FWD(2, 0);
    else DTMX_GC_FWD(2, 1);
  });
#undef DTMX_GC_FWD
  return y;
}

at::Tensor gconv_dgrad(const at::Tensor& dy, const at::Tensor& w, long stride,
                       long pad, long groups, long H, long W_) {
  const char* op = "gconv_dgrad";
  gc_check_act(op, "dy", dy);
  gc_check_sp(op, stride, pad);
  long N = dy.size(0), C = dy.size(1), P, Q;
  long Cg = gc_check_groups(op, C, groups);
  gc_check_w(op, w, dy, Cg);
  TORCH_CHECK(H > 0 && W_ > 0 && gc_out_dims(H, W_, stride, pad, P, Q) &&
                  P == dy.size(2) && Q == dy.size(3),
              "gconv_dgrad: dy spatial size does not match H, W, stride, pad");
  TORCH_CHECK(N * C * H * W_ < (1ll << 31), "gconv_dgrad: dx too large");
  auto dx = at::empty({N, C, H, W_}, dy.options(), at::MemoryFormat::ChannelsLast);
  auto wp = gc_pack(w, C, Cg, true);
  // sub-grid extents of the parity classes: rows a, a + stride, ...
  FastDiv dH0, dW0, dH1, dW1;
  dH0.init((uint32_t)((H + stride - 1) / stride));
  dW0.init((uint32_t)((W_ + stride - 1) / stride));
  // class 1 exists for stride 2 only, and may be empty (H or W == 1): the
  // kernel skips it, the divisor is then a placeholder
  uint32_t h1 = stride == 2 ? (uint32_t)(H / 2) : 0, w1 = stride == 2 ? (uint32_t)(W_ / 2) : 0;
  dH1.init(h1 ? h1 : 1);
  dW1.init(w1 ? w1 : 1);
  dim3 grid = gc_gather_grid(N * (long)dH0.d * (long)dW0.d, C);
#define DTMX_GC_DGRAD(S_, P_)                                                      \
  gconv_gather_kernel<elem_t, S_, P_, true><<<grid, GC_THREADS, 0, gc_stream()>>>(  \
      (const elem_t*)dy.data_ptr(), (const elem_t*)wp.data_ptr(),                  \
      (elem_t*)dx.data_ptr(), N, C, P, Q, H, W_, dH0, dW0, dH1, dW1)
  DTMX_DISPATCH_16(dy.scalar_type(), "gconv_dgrad", {
    if (stride == 1 && pad == 0) DTMX_GC_DGRAD(1, 0);
    else if (stride == 1) DTMX_GC_DGRAD(1, 1);
    else if (pad == 0) DTMX_GC_DGRAD(2, 0);
    else DTMX_GC_DGRAD(2, 1);
  });
#undef DTMX_GC_DGRAD
  return dx;
}

at::Tensor gconv_wgrad(const at::Tensor& x, const at::Tensor& dy, long stride,
                       long pad, long groups, bool w_channels_last) {
  const char* op = "gconv_wgrad";
  gc_check_act(op, "x", x);
  gc_check_act(op, "dy", dy);
  gc_check_sp(op, stride, pad);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.device() == x.device(),
              "gconv_wgrad: x and dy must share dtype and device");
  long N = x.size(0), C = x.size(1), H = x.size(2), W_ = x.size(3), P, Q;
  long Cg = gc_check_groups(op, C, groups);
  TORCH_CHECK(gc_out_dims(H, W_, stride, pad, P, Q) && dy.size(0) == N &&
                  dy.size(1) == C && dy.size(2) == P && dy.size(3) == Q,
              "gconv_wgrad: dy shape does not match x, stride, pad");
  long M = N * P * Q, CT = C / GC_CT;
  uint32_t ksteps = (uint32_t)((M + GC_WG_KT - 1) / GC_WG_KT);
  // pixel slices: enough blocks to fill the machine while a wave keeps a few
  // steps, and the fp32 workspace (NB x 9 x C x Cg) stays under its cap
  long slice_bytes = 9 * C * Cg * 4;
  long NB = (ksteps + GC_WAVES * GC_WG_MIN_STEPS - 1) / (GC_WAVES * GC_WG_MIN_STEPS);
  long cap = std::min<long>(2 * GC_BLOCKS / CT, GC_WG_WS_BYTES / slice_bytes);
  if (NB > cap) NB = cap;
  if (NB < 1) NB = 1;
  auto part = at::empty({NB, 9, C, Cg}, x.options().dtype(at::kFloat));
  auto dw = at::empty({C, Cg, 3, 3}, x.options(),
                      w_channels_last ? at::MemoryFormat::ChannelsLast
                                      : at::MemoryFormat::Contiguous);
  FastDiv dQ, dP;
  dQ.init((uint32_t)Q);
  dP.init((uint32_t)P);
  dim3 grid((uint32_t)NB, (uint32_t)CT);
#define DTMX_GC_WGRAD(S_, F_)                                                      \
  gconv_wgrad_partial_kernel<elem_t, S_, F_><<<grid, GC_THREADS, 0, gc_stream()>>>( \
      (const elem_t*)x.data_ptr(), (const elem_t*)dy.data_ptr(),                   \
      part.data_ptr<float>(), C, Cg, H, W_, M, ksteps, (int)pad, dQ, dP)
  DTMX_DISPATCH_16(x.scalar_type(), "gconv_wgrad", {
    if (stride == 1 && Cg == 32) DTMX_GC_WGRAD(1, true);
    else if (stride == 1) DTMX_GC_WGRAD(1, false);
    else if (Cg == 32) DTMX_GC_WGRAD(2, true);
    else DTMX_GC_WGRAD(2, false);
    uint32_t fb = (uint32_t)((9 * C * Cg + GC_FIN_I - 1) / GC_FIN_I);
    gconv_wgrad_finalize_kernel<elem_t><<<fb, GC_THREADS, 0, gc_stream()>>>(
        part.data_ptr<float>(), (elem_t*)dw.data_ptr(), C, Cg, (uint32_t)NB,
        w_channels_last);
  });
#undef DTMX_GC_WGRAD
  return dw;
}

}  // namespace dtmx
