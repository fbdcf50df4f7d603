// First-layer convolution (fwd / wgrad) for 1..4 input channels, gfx950, NHWC.
// (reference src/operator/nn/convolution.cu on the 3-channel image: the stems
// of ResNet, GoogLeNet, Inception, MobileNet and VGG.)
//
// x is read as stored, C = 1..4 channels per pixel (2C bytes, element
// alignment). Inside LDS a pixel is 4 channels (8 bytes, channels >= C zero),
// so 8 consecutive patch pixels of one input row are 32 contiguous 16-bit
// elements: the K extent of v_mfma_f32_16x16x32. The contraction runs over
// (r, s', c4), s' in [0, 8): one MFMA K step per kernel row, R steps in all
// (224 terms for 7x7 where the 8-channel padded path contracts 392). Weight
// entries with s' >= S or c4 >= C are zero.
//
// A work item is a tile of SC_TP x SC_TQ = 8 x 16 output pixels of one image.
// A block (4 waves) stages the tile's input patch, ((TP-1) stride + R) rows
// by ((TQ-1) stride + 8) pixels, once: raw C-channel pixels are read with
// 2-byte loads, out-of-image pixels are written as zero. No padded copy of x
// exists in HBM. Blocks walk tiles in a grid-stride loop.
//
//   fwd    D[ko][px] += Wp_r[ko][32] . Patch_r[32][px]   per kernel row r.
//          The weight is the A operand and stays in registers for the whole
//          walk (R x 4 fragments per lane); the B fragment of lane l is the 16
//          patch bytes at row p stride + r, pixel q stride + 2 (l >> 4), two
//          8-byte LDS reads. Wave w owns output rows 2w, 2w+1 of the tile.
//          Weight rows are permuted as in gconv.hip, so a lane's 2 x 4
//          accumulators are 8 consecutive output channels: one 16-byte store.
//          With STATS a tile also writes one exclusive fp32 row of sum(y) and
//          sum(y^2) over the rounded values it stored.
//   wgrad  D[ko][(s', c4)] += dY[ko][px] . Xcol_r[px][(s', c4)] contracts over
//          the tile's 128 pixels. dy is staged [128 px][<= 64 ko]; both
//          operands are read pixel-major with ds_read_b64_tr_b16. The Xcol_r
//          row of pixel (p, q) is the patch at (p stride + r, q stride), so
//          rows of adjacent pixels overlap and nothing is copied. Wave w owns
//          output channels 16w .. 16w+15 and all R x 32 columns: 2R
//          accumulators per lane, kept across the block's walk over tiles.
//          Stage 1 writes part[slice][Ko][R][8][4] in fp32, stage 2 sums the
//          slices in a fixed order and writes dw in the parameter's layout.
//
// No atomics anywhere: every output element is written once and results are
// bit-identical run to run. A zero weight column meets the real pixels right
// of the window (s' in [S, 8)): a non-finite input pixel therefore reaches
// outputs up to 8 - S pixels left of the windows that contain it.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "dtmx_common.h"

// The statistics epilogue and the slice sums are plain fp32 arithmetic: keep
// the compiler from pairing it into packed fp32 instructions in this file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace dtmx {

static hipStream_t sc_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int SC_THREADS = 256;  // 4 waves
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_TP = 8, SC_TQ = 16;  // output tile, rows x pixels
constexpr int SC_KT = 64;        // output channels per tile
constexpr int SC_MAXR = 7;       // kernel rows
constexpr int SC_SW = 8;         // kernel columns of one K step (S <= 8)
constexpr int SC_BLOCKS = 1024;  // fwd: target grid size
constexpr int SC_WG_BLOCKS = 2 * DTMX_CUS;   // wgrad: two blocks per CU
constexpr long SC_WG_WS_BYTES = 32l << 20;   // wgrad: workspace cap
constexpr int SC_MAX_SLICES = 4096;
constexpr int SC_FIN_I = 16;     // finalize: outputs per block ...
constexpr int SC_FIN_B = 16;     // ... x partial slices per output
constexpr int SC_DY_BYTES = SC_TP * SC_TQ * SC_KT * 2;  // wgrad dy image

static_assert(SC_TP == 2 * SC_WAVES, "fwd: a wave owns two output rows");
static_assert(SC_KT == 16 * SC_WAVES, "wgrad: a wave owns 16 output channels");
static_assert(SC_FIN_I * SC_FIN_B == SC_THREADS, "finalize block shape");

// patch geometry of one tile: pixels per row, rows at R = SC_MAXR, bytes
template <int STRIDE>
struct ScPatch {
  static constexpr int PW = (SC_TQ - 1) * STRIDE + SC_SW;
  static constexpr int MAXROWS = (SC_TP - 1) * STRIDE + SC_MAXR;
  static constexpr int BYTES = MAXROWS * PW * 8;
  static constexpr int NIT = (MAXROWS * PW + SC_THREADS - 1) / SC_THREADS;
};

typedef __attribute__((ext_vector_type(2))) unsigned int sc_u32x2;

// ------------------------------------------------------------- weight pack

// wp[ko][r][s'][c4], s' in [0, 8), c4 in [0, 4): zero where s' >= S or
// c4 >= C. Thread i = (ko, r, s') writes one 8-byte pixel. The weight is read
// through its strides, so both dense layouts of (Ko, C, R, S) pack alike.
template <typename elem_t>
__global__ __launch_bounds__(SC_THREADS) void stemconv_pack_kernel(
    const elem_t* __restrict__ w, elem_t* __restrict__ wp, uint32_t total,
    uint32_t C, uint32_t R, uint32_t S, long s0, long s1, long s2, long s3) {
  uint32_t i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= total) return;
  uint32_t sp = i & 7, t = i >> 3;
  uint32_t ko = t / R, r = t - ko * R;
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) {
    elem_t e = (elem_t)0.f;
    if (sp < S && c < C) e = w[(long)ko * s0 + (long)c * s1 + (long)r * s2 + (long)sp * s3];
    wp[(size_t)i * 4 + c] = e;
  }
}

// ------------------------------------------------------------ tile helpers

struct ScTile {
  uint32_t n, p0, q0;
};

__device__ __forceinline__ ScTile sc_tile(uint32_t t, FastDiv dTQ, FastDiv dTP) {
  uint32_t u = dTQ.div(t), tq = dTQ.mod(t, u);
  uint32_t n = dTP.div(u), tp = dTP.mod(u, n);
  return ScTile{n, tp * SC_TP, tq * SC_TQ};
}

// Stages the patch of tile `tl`: rows (p0 stride - ph) .. + prows, pixels
// (q0 stride - pw) .. + PW, each as 4 channels. All loads of a thread are
// issued before its first LDS write. The caller brackets it with barriers.
template <int STRIDE>
__device__ __forceinline__ void sc_stage_patch(
    const unsigned short* __restrict__ x, char* patch, ScTile tl, uint32_t C,
    uint32_t H, uint32_t W, uint32_t prows, int ph, int pw) {
  using G = ScPatch<STRIDE>;
  const int ih0 = (int)(tl.p0 * STRIDE) - ph, iw0 = (int)(tl.q0 * STRIDE) - pw;
  const uint32_t npix = prows * G::PW;
  s16x4 v[G::NIT];
#pragma unroll
  for (int it = 0; it < G::NIT; ++it) {
    const uint32_t idx = threadIdx.x + it * SC_THREADS;
    const uint32_t row = idx / G::PW, col = idx - row * G::PW;
    const int ih = ih0 + (int)row, iw = iw0 + (int)col;
    v[it] = s16x4{0, 0, 0, 0};
    if (idx < npix && (uint32_t)ih < H && (uint32_t)iw < W) {
      const unsigned short* src =
          x + (((size_t)tl.n * H + (uint32_t)ih) * W + (uint32_t)iw) * C;
      v[it][0] = (short)src[0];
      if (C > 1) v[it][1] = (short)src[1];
      if (C > 2) v[it][2] = (short)src[2];
      if (C > 3) v[it][3] = (short)src[3];
    }
  }
#pragma unroll
  for (int it = 0; it < G::NIT; ++it) {
    const uint32_t idx = threadIdx.x + it * SC_THREADS;
    if (idx < npix) *(s16x4*)(patch + idx * 8) = v[it];
  }
}

// ------------------------------------------------------------------ forward

// grid = (tile walkers, Ko tiles of 64). Lane l = (i = l & 15, g = l >> 4).
// Fragment m = 2 pr + nh of kernel row r is the A operand of the MFMA that
// yields channels kt 64 + 32 pr + 8 g' + 4 nh + e in accumulator register e of
// lane group g': A row i is channel 32 pr + 8 (i >> 2) + 4 nh + (i & 3).
template <typename elem_t, int STRIDE, bool STATS>
__global__ __launch_bounds__(SC_THREADS, 2) void stemconv_fwd_kernel(
    const unsigned short* __restrict__ x, const elem_t* __restrict__ wp,
    elem_t* __restrict__ y, float* __restrict__ psum, float* __restrict__ psumsq,
    uint32_t C, uint32_t H, uint32_t W, uint32_t Ko, uint32_t R, uint32_t P,
    uint32_t Q, int ph, int pw, uint32_t tiles, FastDiv dTQ, FastDiv dTP) {
  using V8 = typename E8<elem_t>::v8;
  using G = ScPatch<STRIDE>;
  union Frag {
    V8 v;
    s16x4 h[2];
  };
  __shared__ __attribute__((aligned(16))) char patch[G::BYTES];
  __shared__ float red[STATS ? 2 * SC_WAVES * SC_KT : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t i = lane & 15, g = lane >> 4;
  const uint32_t kbase = blockIdx.y * SC_KT;
  const bool two = Ko - kbase > 32;  // the tile has a second 32-channel pair
  const uint32_t prows = (SC_TP - 1) * STRIDE + R;

  V8 wf[SC_MAXR][4];
#pragma unroll
  for (int r = 0; r < SC_MAXR; ++r)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t ch = kbase + 32 * (m >> 1) + 8 * (i >> 2) + 4 * (m & 1) + (i & 3);
      V8 f;
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = (elem_t)0.f;
      if ((uint32_t)r < R && ch < Ko)
        f = *(const V8*)(wp + ((size_t)ch * R + r) * 32 + 8 * g);
      wf[r][m] = f;
    }

  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const ScTile tl = sc_tile(t, dTQ, dTP);
    __syncthreads();  // the previous tile's fragment reads are done
    sc_stage_patch<STRIDE>(x, patch, tl, C, H, W, prows, ph, pw);
    __syncthreads();

    f32x4 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[mt][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < SC_MAXR; ++r) {
      if ((uint32_t)r >= R) break;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const uint32_t prow = (2 * wv + mt) * STRIDE + r;
        const char* a = patch + (prow * G::PW + i * STRIDE + 2 * g) * 8;
        Frag b;
        b.h[0] = *(const s16x4*)a;
        b.h[1] = *(const s16x4*)(a + 8);
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m < 2 || two) acc[mt][m] = E8<elem_t>::mfma(wf[r][m], b.v, acc[mt][m]);
      }
    }

    // lane (i, g) holds channels 8g .. 8g+7 of each pair for pixel q0 + i of
    // rows p0 + 2 wv + mt
    const uint32_t q = tl.q0 + i;
    float s[2][8], ss[2][8];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr)
#pragma unroll
      for (int e = 0; e < 8; ++e) s[pr][e] = ss[pr][e] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const uint32_t p = tl.p0 + 2 * wv + mt;
      const bool live = p < P && q < Q;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const uint32_t coff = kbase + 32 * pr + 8 * g;
        V8 o;
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
          for (int e = 0; e < 4; ++e) o[4 * nh + e] = (elem_t)acc[mt][2 * pr + nh][e];
        if (live && coff < Ko) {
          *(V8*)(y + (((size_t)tl.n * P + p) * Q + q) * Ko + coff) = o;
          if (STATS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float f = (float)o[e];
              s[pr][e] += f;
              ss[pr][e] += f * f;
            }
          }
        }
      }
    }
    if (STATS) {
      // fold the 16 pixels of a lane group, then the 4 waves in wave order
#pragma unroll
      for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int d = 1; d < 16; d <<= 1) {
            s[pr][e] += __shfl_xor(s[pr][e], d);
            ss[pr][e] += __shfl_xor(ss[pr][e], d);
          }
      if (i == 0) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            red[wv * SC_KT + 32 * pr + 8 * g + e] = s[pr][e];
            red[(SC_WAVES + wv) * SC_KT + 32 * pr + 8 * g + e] = ss[pr][e];
          }
      }
      __syncthreads();
      if (tid < SC_KT && kbase + tid < Ko) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w_ = 0; w_ < SC_WAVES; ++w_) {
          a += red[w_ * SC_KT + tid];
          b += red[(SC_WAVES + w_) * SC_KT + tid];
        }
        psum[(size_t)t * Ko + kbase + tid] = a;
        psumsq[(size_t)t * Ko + kbase + tid] = b;
      }
    }
  }
}

// -------------------------------------------------------------------- wgrad

// One transposed read: the 16 lanes of a group each supply the address of 4
// consecutive 16-bit elements (lane 4 a + b: row a, elements 4b .. 4b+3 of a
// [4][16] block) and lane c receives column c of the four rows.
__device__ __forceinline__ void sc_tr4(unsigned a0, unsigned a1, unsigned a2,
                                       unsigned a3, sc_u32x2 (&t)[4]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);  // keep the MFMAs below the asm's wait
}

__device__ __forceinline__ void sc_tr2(unsigned a0, unsigned a1, sc_u32x2 (&t)[2]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(t[0]), "=&v"(t[1])
      : "v"(a0), "v"(a1)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Stage 1. grid = (slices, Ko tiles of 64). Slice s walks tiles
// [s per, (s + 1) per) and keeps D[16 ko per wave][R][32] in registers.
//
// dy image: pixel px = 16 prow + qq of the tile, channel ch of the Ko tile at
// byte (px >> 3) 1024 + ((ch >> 3) 8 + (px & 7)) 16 + (ch & 7) 2: the 8 pixels
// of a transposed-read pair are 16 bytes apart, so a group's 16 lanes cover
// 2 x 64 consecutive bytes. Tail pixels and channels >= Ko are staged as zero.
// K step ks covers px 32 ks .. + 31; lane group g holds px 32 ks + 8 g + j.
template <typename elem_t, int STRIDE>
__global__ __launch_bounds__(SC_THREADS, 2) void stemconv_wgrad_partial_kernel(
    const unsigned short* __restrict__ x, const elem_t* __restrict__ dy,
    float* __restrict__ part, uint32_t C, uint32_t H, uint32_t W, uint32_t Ko,
    uint32_t R, uint32_t P, uint32_t Q, int ph, int pw, uint32_t tiles,
    uint32_t per, FastDiv dTQ, FastDiv dTP) {
  using V8 = typename E8<elem_t>::v8;
  using G = ScPatch<STRIDE>;
  union Frag {
    V8 v;
    sc_u32x2 h[2];
  };
  __shared__ __attribute__((aligned(16))) char patch[G::BYTES];
  __shared__ __attribute__((aligned(16))) char dyimg[SC_DY_BYTES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t i = lane & 15, g = lane >> 4;
  const uint32_t kbase = blockIdx.y * SC_KT;
  const bool active = kbase + 16 * wv < Ko;  // whole wave
  const uint32_t prows = (SC_TP - 1) * STRIDE + R;

  f32x4 acc[SC_MAXR][2];
#pragma unroll
  for (int r = 0; r < SC_MAXR; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[r][h] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint32_t t0 = blockIdx.x * per;
  const uint32_t t1 = t0 + per < tiles ? t0 + per : tiles;
  for (uint32_t t = t0; t < t1; ++t) {
    const ScTile tl = sc_tile(t, dTQ, dTP);
    __syncthreads();  // the previous tile's fragment reads are done
    sc_stage_patch<STRIDE>(x, patch, tl, C, H, W, prows, ph, pw);
    {
      V8 v[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const uint32_t c = tid + it * SC_THREADS;  // 16-byte piece of the image
        const uint32_t px = (c >> 6) * 8 + (c & 7), ch = kbase + ((c >> 3) & 7) * 8;
        const uint32_t p = tl.p0 + (px >> 4), q = tl.q0 + (px & 15);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[it][e] = (elem_t)0.f;
        if (p < P && q < Q && ch < Ko)
          v[it] = *(const V8*)(dy + (((size_t)tl.n * P + p) * Q + q) * Ko + ch);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it)
        *(V8*)(dyimg + (tid + it * SC_THREADS) * 16) = v[it];
    }
    __syncthreads();
    if (!active) continue;

    const unsigned dybase = (unsigned)(uintptr_t)dyimg + g * 1024 +
                            ((2 * wv + ((i & 3) >> 1)) * 8 + (i >> 2)) * 16 +
                            (i & 1) * 8;
    // patch pixel of lane i for the group's pixel j = i >> 2 (+ 4 for the
    // second read), column half 0, kernel row 0, K step 0
    const unsigned xbase =
        (unsigned)(uintptr_t)patch +
        (((g >> 1) * STRIDE) * G::PW + (8 * (g & 1) + (i >> 2)) * STRIDE + (i & 3)) * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Frag a;
      {
        sc_u32x2 tr[2];
        const unsigned d0 = dybase + ks * 4096;
        sc_tr2(d0, d0 + 64, tr);
        a.h[0] = tr[0];
        a.h[1] = tr[1];
      }
#pragma unroll
      for (int r = 0; r < SC_MAXR; ++r) {
        if ((uint32_t)r >= R) break;
        const unsigned x0 = xbase + ((2 * ks * STRIDE + r) * G::PW) * 8;
        sc_u32x2 tr[4];
        sc_tr4(x0, x0 + 4 * STRIDE * 8, x0 + 32, x0 + 4 * STRIDE * 8 + 32, tr);
        Frag b0, b1;
        b0.h[0] = tr[0];
        b0.h[1] = tr[1];
        b1.h[0] = tr[2];
        b1.h[1] = tr[3];
        acc[r][0] = E8<elem_t>::mfma(a.v, b0.v, acc[r][0]);
        acc[r][1] = E8<elem_t>::mfma(a.v, b1.v, acc[r][1]);
      }
    }
  }

  // D row 4 g + e is channel kbase + 16 wv + 4 g + e, column i of half h is
  // (s' = 4 h + (i >> 2), c4 = i & 3)
#pragma unroll
  for (int r = 0; r < SC_MAXR; ++r) {
    if ((uint32_t)r >= R) break;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t ko = kbase + 16 * wv + 4 * g + e;
        if (ko < Ko)
          part[(((size_t)blockIdx.x * Ko + ko) * R + r) * 32 + 16 * h + i] = acc[r][h][e];
      }
  }
}

// Stage 2. Output o = ((ko C + c) R + r) S + s sums part[0 .. NB) in a fixed
// order, converts once and lands in dw's layout: [Ko][C][R][S], or
// [Ko][R][S][C] when w_cl. A block is SC_FIN_I outputs x SC_FIN_B slices.
template <typename elem_t>
__global__ __launch_bounds__(SC_THREADS) void stemconv_wgrad_finalize_kernel(
    const float* __restrict__ part, elem_t* __restrict__ dw, uint32_t Ko,
    uint32_t C, uint32_t R, uint32_t S, uint32_t NB, bool w_cl) {
  __shared__ float red[SC_FIN_B][SC_FIN_I];
  const uint32_t il = threadIdx.x % SC_FIN_I, b = threadIdx.x / SC_FIN_I;
  const uint32_t o = blockIdx.x * SC_FIN_I + il;
  const uint32_t n = Ko * C * R * S;
  const uint32_t oo = o < n ? o : 0;
  uint32_t s = oo % S, u = oo / S;
  uint32_t r = u % R;
  u /= R;
  uint32_t c = u % C, ko = u / C;
  const size_t slice = (size_t)Ko * R * 32;
  const size_t src = ((size_t)ko * R + r) * 32 + s * 4 + c;
  float v = 0.f;
  if (o < n)
    for (uint32_t k = b; k < NB; k += SC_FIN_B) v += part[k * slice + src];
  red[b][il] = v;
  __syncthreads();
  if (b == 0 && o < n) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < SC_FIN_B; ++k) tot += red[k][il];
    const size_t dst = w_cl ? (((size_t)ko * R + r) * S + s) * C + c : (size_t)o;
    dw[dst] = (elem_t)tot;
  }
}

// --------------------------------------------------------------- host side

struct ScShape {
  long N, C, H, W, Ko, R, S, P, Q, tiles_p, tiles_q;
};

// logical NCHW with channels_last strides; size-1 dims may carry any stride
static bool sc_is_nhwc(const at::Tensor& t) {
  long C = t.size(1), H = t.size(2), W = t.size(3);
  long want[4] = {H * W * C, 1, W * C, C};
  for (int d = 0; d < 4; ++d)
    if (t.size(d) > 1 && t.stride(d) != want[d]) return false;
  return true;
}

static ScShape sc_check(const char* op, const at::Tensor& x, long Ko, long R, long S,
                        long stride, long ph, long pw) {
  TORCH_CHECK(x.is_cuda() && (x.scalar_type() == at::kBFloat16 ||
                              x.scalar_type() == at::kHalf),
              op, ": x must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && sc_is_nhwc(x), op,
              ": x must be a non-empty 4-D NHWC (channels_last) tensor");
  ScShape s;
  s.N = x.size(0); s.C = x.size(1); s.H = x.size(2); s.W = x.size(3);
  s.Ko = Ko; s.R = R; s.S = S;
  TORCH_CHECK(s.C >= 1 && s.C <= 4, op, ": 1 <= C <= 4 required, got C = ", s.C);
  TORCH_CHECK(Ko > 0 && Ko % 8 == 0, op, ": Ko % 8 == 0 required, got Ko = ", Ko);
  TORCH_CHECK(R >= 1 && R <= SC_MAXR, op, ": 1 <= R <= 7 required, got R = ", R);
  TORCH_CHECK(S >= 1 && S <= SC_SW, op, ": 1 <= S <= 8 required, got S = ", S);
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ", stride);
  TORCH_CHECK(ph >= 0 && ph < R, op, ": 0 <= pad_h < R required, got ", ph);
  TORCH_CHECK(pw >= 0 && pw < S, op, ": 0 <= pad_w < S required, got ", pw);
  TORCH_CHECK(s.H + 2 * ph >= R && s.W + 2 * pw >= S, op,
              ": input smaller than the window (empty output)");
  s.P = (s.H + 2 * ph - R) / stride + 1;
  s.Q = (s.W + 2 * pw - S) / stride + 1;
  // offsets are 64-bit; the 32-bit quantities are x's elements and y's pixels
  // (the bs4096 ResNet stem writes 3.3e9 elements)
  TORCH_CHECK(x.numel() < (1ll << 31), op, ": x too large (>= 2^31 elements)");
  TORCH_CHECK(s.N * s.P * s.Q < (1ll << 31), op, ": y too large (>= 2^31 pixels)");
  s.tiles_p = (s.P + SC_TP - 1) / SC_TP;
  s.tiles_q = (s.Q + SC_TQ - 1) / SC_TQ;
  return s;
}

static at::Tensor sc_pack(const char* op, const at::Tensor& w, const at::Tensor& x) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == x.scalar_type() &&
                  w.device() == x.device(),
              op, ": w must be on the device of x and of its dtype");
  TORCH_CHECK(w.dim() == 4 && w.numel() > 0 && w.size(1) == x.size(1), op,
              ": w must be a non-empty (Ko, C, R, S) tensor with the C of x");
  TORCH_CHECK(w.is_contiguous() || w.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": weight memory must be dense [Ko][C][R][S] or [Ko][R][S][C]");
  const long Ko = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  auto wp = at::empty({Ko, R, 32}, w.options());
  const uint32_t total = (uint32_t)(Ko * R * 8);
  DTMX_DISPATCH_16(w.scalar_type(), "stemconv_pack", {
    stemconv_pack_kernel<elem_t>
        <<<(total + SC_THREADS - 1) / SC_THREADS, SC_THREADS, 0, sc_stream()>>>(
            (const elem_t*)w.data_ptr(), (elem_t*)wp.data_ptr(), total, (uint32_t)C,
            (uint32_t)R, (uint32_t)S, w.stride(0), w.stride(1), w.stride(2),
            w.stride(3));
  });
  return wp;
}

std::vector<at::Tensor> stemconv_fwd(const at::Tensor& x, const at::Tensor& w,
                                     long stride, long ph, long pw, bool want_stats) {
  const char* op = "stemconv_fwd";
  TORCH_CHECK(w.dim() == 4, op, ": w must be a (Ko, C, R, S) tensor");
  const ScShape s = sc_check(op, x, w.size(0), w.size(2), w.size(3), stride, ph, pw);
  TORCH_CHECK(w.numel() < (1ll << 31), op, ": w too large (>= 2^31 elements)");
  auto wp = sc_pack(op, w, x);
  auto y = at::empty({s.N, s.Ko, s.P, s.Q}, x.options(), at::MemoryFormat::ChannelsLast);
  const long tiles = s.N * s.tiles_p * s.tiles_q;
  const auto opt_f = x.options().dtype(at::kFloat);
  auto psum = at::empty({want_stats ? tiles : 0, want_stats ? s.Ko : 0}, opt_f);
  auto psumsq = at::empty_like(psum);
  FastDiv dTQ, dTP;
  dTQ.init((uint32_t)s.tiles_q);
  dTP.init((uint32_t)s.tiles_p);
  const uint32_t gy = (uint32_t)((s.Ko + SC_KT - 1) / SC_KT);
  const long cap = std::max<long>(1, SC_BLOCKS / gy);
  dim3 grid((uint32_t)std::min(tiles, cap), gy);
#define DTMX_SC_FWD(S_, ST_)                                                       \
  stemconv_fwd_kernel<elem_t, S_, ST_><<<grid, SC_THREADS, 0, sc_stream()>>>(      \
      (const unsigned short*)x.data_ptr(), (const elem_t*)wp.data_ptr(),           \
      (elem_t*)y.data_ptr(), psum.data_ptr<float>(), psumsq.data_ptr<float>(),     \
      (uint32_t)s.C, (uint32_t)s.H, (uint32_t)s.W, (uint32_t)s.Ko, (uint32_t)s.R,  \
      (uint32_t)s.P, (uint32_t)s.Q, (int)ph, (int)pw, (uint32_t)tiles, dTQ, dTP)
  DTMX_DISPATCH_16(x.scalar_type(), op, {
    if (stride == 1 && !want_stats) DTMX_SC_FWD(1, false);
    else if (stride == 1) DTMX_SC_FWD(1, true);
    else if (!want_stats) DTMX_SC_FWD(2, false);
    else DTMX_SC_FWD(2, true);
  });
#undef DTMX_SC_FWD
  return {y, psum, psumsq};
}

at::Tensor stemconv_wgrad(const at::Tensor& x, const at::Tensor& dy, long R, long S,
                          long stride, long ph, long pw, bool w_channels_last,
                          long slices) {
  const char* op = "stemconv_wgrad";
  TORCH_CHECK(dy.dim() == 4, op, ": dy must be a 4-D NHWC tensor");
  const ScShape s = sc_check(op, x, dy.size(1), R, S, stride, ph, pw);
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == x.scalar_type() &&
                  dy.device() == x.device(),
              op, ": x and dy must share dtype and device");
  TORCH_CHECK(dy.size(0) == s.N && dy.size(2) == s.P && dy.size(3) == s.Q, op,
              ": dy shape does not match x, the window, stride and padding");
  TORCH_CHECK(sc_is_nhwc(dy), op, ": dy must be channels_last (NHWC) in memory");
  TORCH_CHECK(((uintptr_t)dy.data_ptr() & 15) == 0, op, ": dy must be 16-byte aligned");
  TORCH_CHECK(slices >= 0 && slices <= SC_MAX_SLICES, op,
              ": 0 <= slices <= ", SC_MAX_SLICES, " required, got ", slices);
  const long tiles = s.N * s.tiles_p * s.tiles_q;
  const long gy = (s.Ko + SC_KT - 1) / SC_KT;
  const long slice_bytes = s.Ko * R * 32 * 4;
  // slices = blocks per Ko tile: two blocks per CU while the fp32 workspace
  // stays under its cap; then only as many as have tiles to walk
  long NB = slices, per;
  if (NB == 0) {
    NB = std::min<long>(SC_WG_BLOCKS / gy, SC_WG_WS_BYTES / slice_bytes);
    NB = std::max<long>(1, std::min(NB, tiles));
    per = (tiles + NB - 1) / NB;
    NB = (tiles + per - 1) / per;
  } else {
    per = (tiles + NB - 1) / NB;
  }
  auto part = at::empty({NB, s.Ko, R, 32}, x.options().dtype(at::kFloat));
  auto dw = at::empty({s.Ko, s.C, R, S}, x.options(),
                      w_channels_last ? at::MemoryFormat::ChannelsLast
                                      : at::MemoryFormat::Contiguous);
  FastDiv dTQ, dTP;
  dTQ.init((uint32_t)s.tiles_q);
  dTP.init((uint32_t)s.tiles_p);
  dim3 grid((uint32_t)NB, (uint32_t)gy);
#define DTMX_SC_WGRAD(S_)                                                          \
  stemconv_wgrad_partial_kernel<elem_t, S_><<<grid, SC_THREADS, 0, sc_stream()>>>( \
      (const unsigned short*)x.data_ptr(), (const elem_t*)dy.data_ptr(),           \
      part.data_ptr<float>(), (uint32_t)s.C, (uint32_t)s.H, (uint32_t)s.W,         \
      (uint32_t)s.Ko, (uint32_t)R, (uint32_t)s.P, (uint32_t)s.Q, (int)ph, (int)pw, \
      (uint32_t)tiles, (uint32_t)per, dTQ, dTP)
  DTMX_DISPATCH_16(x.scalar_type(), op, {
    if (stride == 1) DTMX_SC_WGRAD(1);
    else DTMX_SC_WGRAD(2);
    const uint32_t n = (uint32_t)(s.Ko * s.C * R * S);
    stemconv_wgrad_finalize_kernel<elem_t>
        <<<(n + SC_FIN_I - 1) / SC_FIN_I, SC_THREADS, 0, sc_stream()>>>(
            part.data_ptr<float>(), (elem_t*)dw.data_ptr(), (uint32_t)s.Ko,
            (uint32_t)s.C, (uint32_t)R, (uint32_t)S, (uint32_t)NB, w_channels_last);
  });
#undef DTMX_SC_WGRAD
  return dw;
}

}  // namespace dtmx

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
