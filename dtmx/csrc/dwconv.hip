// Depthwise 3x3 convolution (fwd / dgrad / wgrad) for gfx950, NHWC.
// (reference src/operator/nn/depthwise_convolution_tf.cuh — the depthwise
// special case mobilenet v1/v2 spend every second conv in.)
//
// groups == C_in == C_out, multiplier 1: no GEMM, one input channel per
// output channel — a pure bandwidth op. One thread owns a bf16x8/f16x8
// channel vector (16-B loads/stores, lanes walk C first so a wave reads
// whole NHWC rows) and a short strip of outputs along W, so the input
// columns neighbouring outputs share are read once into registers.
// The nine taps of the thread's 8 channels live in registers as fp32.
// Weight memory is the parameter as stored: [C][3][3].
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"

namespace dtmx {

static hipStream_t dw_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int DW_THREADS = 256;
constexpr int DW_STRIP = 4;       // outputs per thread along W (fwd, dgrad, wgrad)
constexpr int DW_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; grid-stride the rest
constexpr int DW_WG_CVB = 32;     // wgrad: channel vectors per block (<= 256/8)
constexpr int DW_WG_BLOCKS = 1024;   // wgrad: target partial-producing blocks
constexpr int DW_FIN_I = 16;      // finalize: outputs per block ...
constexpr int DW_FIN_B = 16;      // ... x partial slices per output

static_assert(DW_STRIP % 2 == 0, "stride-2 dgrad parity needs an even strip");
static_assert(DW_WG_CVB * 8 <= DW_THREADS, "wgrad block reduce: one thread per channel");
static_assert(DW_FIN_I * DW_FIN_B == DW_THREADS, "finalize block shape");

template <typename elem_t>
__device__ __forceinline__ typename E8<elem_t>::v8 dw_zero() {
  typename E8<elem_t>::v8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (elem_t)0.f;
  return z;
}

// 8 channels x 9 taps are 72 contiguous elements at w + cv*72 ([C][3][3]):
// nine 16-B loads, then a compile-time register transpose to wt[tap][ch].
template <typename elem_t>
__device__ __forceinline__ void dw_load_taps(const elem_t* __restrict__ w,
                                             uint32_t cv, float (&wt)[9][8]) {
  using V8 = typename E8<elem_t>::v8;
  const V8* src = (const V8*)(w + (size_t)cv * 72);
  V8 raw[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) raw[i] = src[i];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t][e] = (float)raw[(e * 9 + t) >> 3][(e * 9 + t) & 7];
}

// ------------------------------------------------------------------ forward

// work item = (n, p, q-strip, c8), c8 fastest. Padding by predication.
template <typename elem_t, int STRIDE>
__global__ __launch_bounds__(DW_THREADS) void dwconv_fwd_kernel(
    const elem_t* __restrict__ x, const elem_t* __restrict__ w,
    elem_t* __restrict__ y, uint32_t C, uint32_t H, uint32_t W, uint32_t P,
    uint32_t Q, int pad, uint32_t total, FastDiv dCv, FastDiv dQs, FastDiv dP) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int S = DW_STRIP;
  constexpr int NCOL = (S - 1) * STRIDE + 3;
  const uint32_t step = gridDim.x * DW_THREADS;
  float wt[9][8];
  uint32_t cur = 0xffffffffu;  // taps reload only when the channel vector changes
  for (uint32_t i = blockIdx.x * DW_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dQs.div(m), qs = dQs.mod(m, r);
    uint32_t n = dP.div(r), p = dP.mod(r, n);
    if (cv != cur) {
      dw_load_taps<elem_t>(w, cv, wt);
      cur = cv;
    }
    float acc[S][8];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    const int ih0 = (int)(p * STRIDE) - pad;
    const int iw0 = (int)(qs * S * STRIDE) - pad;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int ih = ih0 + kh;
      if ((uint32_t)ih >= H) continue;
      const elem_t* row = x + ((size_t)n * H + (uint32_t)ih) * W * C + cv * 8;
      V8 col[NCOL];
#pragma unroll
      for (int c = 0; c < NCOL; ++c) {
        int iw = iw0 + c;
        col[c] = (uint32_t)iw < W ? *(const V8*)(row + (size_t)(uint32_t)iw * C)
                                  : dw_zero<elem_t>();
      }
#pragma unroll
      for (int j = 0; j < S; ++j)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc[j][e] += (float)col[j * STRIDE + kw][e] * wt[kh * 3 + kw][e];
    }
    elem_t* out = y + (((size_t)n * P + p) * Q + qs * S) * C + cv * 8;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (qs * S + j >= Q) break;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (elem_t)acc[j][e];
      *(V8*)(out + (size_t)j * C) = o;
    }
  }
}

// -------------------------------------------------------------------- dgrad

// Gather form: dx[n,h,w] = sum over taps (kh,kw) with (h+pad-kh, w+pad-kw)
// divisible by the stride and the quotient (p,q) inside dy, of
// dy[n,p,q] * w[kh][kw]. Every dx element is written (zero where no output
// reaches it); no atomics, no zero fill. work item = (n, h, w-strip, c8).
// For stride 2 the strip start is even, so column parity — which taps
// contribute and which dy column they read — is a compile-time function of
// (PAD, j, kw); row parity is a per-thread skip of whole dy rows.
template <typename elem_t, int STRIDE, int PAD>
__global__ __launch_bounds__(DW_THREADS) void dwconv_dgrad_kernel(
    const elem_t* __restrict__ dy, const elem_t* __restrict__ w,
    elem_t* __restrict__ dx, uint32_t C, uint32_t H, uint32_t W, uint32_t P,
    uint32_t Q, uint32_t total, FastDiv dCv, FastDiv dWs, FastDiv dH) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int S = DW_STRIP;
  // dy columns one strip touches, relative to column qb:
  //   stride 1: q = w0 + PAD - 2 + c,  c = j - kw + 2          in [0, S+2)
  //   stride 2: q = w0/2 - 1 + c,      c = ((PAD+j-kw) >> 1) + 1 in [0, S/2+2)
  constexpr int NCOL = STRIDE == 1 ? S + 2 : S / 2 + 2;
  const uint32_t step = gridDim.x * DW_THREADS;
  float wt[9][8];
  uint32_t cur = 0xffffffffu;
  for (uint32_t i = blockIdx.x * DW_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dWs.div(m), ws = dWs.mod(m, r);
    uint32_t n = dH.div(r), h = dH.mod(r, n);
    if (cv != cur) {
      dw_load_taps<elem_t>(w, cv, wt);
      cur = cv;
    }
    float acc[S][8];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    const int w0 = (int)(ws * S);
    const int qb = STRIDE == 1 ? w0 + PAD - 2 : w0 / 2 - 1;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int t = (int)h + PAD - kh;
      if (t < 0) continue;
      if (STRIDE == 2 && (t & 1)) continue;
      uint32_t p = (uint32_t)t / STRIDE;
      if (p >= P) continue;
      const elem_t* row = dy + ((size_t)n * P + p) * Q * C + cv * 8;
      V8 col[NCOL];
#pragma unroll
      for (int c = 0; c < NCOL; ++c) {
        int q = qb + c;
        col[c] = (uint32_t)q < Q ? *(const V8*)(row + (size_t)(uint32_t)q * C)
                                 : dw_zero<elem_t>();
      }
#pragma unroll
      for (int j = 0; j < S; ++j)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int tt = PAD + j - kw;  // column offset from w0, in input units
          if (STRIDE == 2 && (tt & 1)) continue;
          const int c = STRIDE == 1 ? j - kw + 2 : (tt >> 1) + 1;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc[j][e] += (float)col[c][e] * wt[kh * 3 + kw][e];
        }
    }
    elem_t* out = dx + (((size_t)n * H + h) * W + (uint32_t)w0) * C + cv * 8;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if ((uint32_t)w0 + j >= W) break;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (elem_t)acc[j][e];
      *(V8*)(out + (size_t)j * C) = o;
    }
  }
}

// -------------------------------------------------------------------- wgrad

// Stage 1. grid = (NB, channel groups). A block's 256 threads are
// (position lane pl) x (channel vector cvl) with cvl fastest; each thread
// walks output strips (n, p, q-strip) NB*PL apart and keeps 9 taps x 8
// channels of fp32 sums in registers. The block then folds its position
// lanes through LDS in a fixed order and writes part[blockIdx.x][9][C] —
// every element of the workspace is written, so it needs no zero fill.
template <typename elem_t, int STRIDE>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_partial_kernel(
    const elem_t* __restrict__ x, const elem_t* __restrict__ dy,
    float* __restrict__ part, uint32_t C, uint32_t H, uint32_t W, uint32_t P,
    uint32_t Q, int pad, uint32_t nstrips, uint32_t cvb, uint32_t PL,
    FastDiv dQs, FastDiv dP) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int S = DW_STRIP;
  constexpr int NCOL = (S - 1) * STRIDE + 3;
  __shared__ float red[DW_THREADS * 8];
  const uint32_t tid = threadIdx.x;
  const uint32_t pl = tid / cvb, cvl = tid - pl * cvb;
  const uint32_t cv = blockIdx.y * cvb + cvl;
  const bool active = pl < PL && cv * 8 < C;
  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
  if (active) {
    const uint32_t step = gridDim.x * PL;
    for (uint32_t s = blockIdx.x * PL + pl; s < nstrips; s += step) {
      uint32_t r = dQs.div(s), qs = dQs.mod(s, r);
      uint32_t n = dP.div(r), p = dP.mod(r, n);
      const elem_t* gy = dy + (((size_t)n * P + p) * Q + qs * S) * C + cv * 8;
      V8 g[S];
#pragma unroll
      for (int j = 0; j < S; ++j)
        g[j] = qs * S + j < Q ? *(const V8*)(gy + (size_t)j * C) : dw_zero<elem_t>();
      const int ih0 = (int)(p * STRIDE) - pad;
      const int iw0 = (int)(qs * S * STRIDE) - pad;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        int ih = ih0 + kh;
        if ((uint32_t)ih >= H) continue;
        const elem_t* row = x + ((size_t)n * H + (uint32_t)ih) * W * C + cv * 8;
        V8 col[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
          int iw = iw0 + c;
          col[c] = (uint32_t)iw < W ? *(const V8*)(row + (size_t)(uint32_t)iw * C)
                                    : dw_zero<elem_t>();
        }
#pragma unroll
        for (int j = 0; j < S; ++j)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int e = 0; e < 8; ++e)
              acc[kh * 3 + kw][e] += (float)col[j * STRIDE + kw][e] * (float)g[j][e];
      }
    }
  }
  // fixed-order fold over position lanes, one tap at a time (8 KB of LDS)
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[t][e];
    __syncthreads();
    if (tid < cvb * 8) {
      uint32_t c = blockIdx.y * cvb * 8 + tid;
      if (c < C) {
        float s = 0.f;
        for (uint32_t l = 0; l < PL; ++l) s += red[l * cvb * 8 + tid];
        part[((size_t)blockIdx.x * 9 + t) * C + c] = s;
      }
    }
    __syncthreads();
  }
}

// Stage 2. Sums part[0..NB) for each of the 9*C outputs in a fixed order and
// converts. A block is DW_FIN_I outputs x DW_FIN_B slices: slice b adds
// partials b, b+DW_FIN_B, ... ; the slices are then added in slice order.
template <typename elem_t>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_finalize_kernel(
    const float* __restrict__ part, elem_t* __restrict__ dw, uint32_t C,
    uint32_t NB) {
  __shared__ float red[DW_FIN_B][DW_FIN_I];
  const uint32_t il = threadIdx.x % DW_FIN_I, b = threadIdx.x / DW_FIN_I;
  const uint32_t i = blockIdx.x * DW_FIN_I + il;  // index into [9][C]
  const uint32_t n9c = 9 * C;
  float s = 0.f;
  if (i < n9c)
    for (uint32_t k = b; k < NB; k += DW_FIN_B) s += part[(size_t)k * n9c + i];
  red[b][il] = s;
  __syncthreads();
  if (b == 0 && i < n9c) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < DW_FIN_B; ++k) tot += red[k][il];
    uint32_t t = i / C, c = i - t * C;
    dw[(size_t)c * 9 + t] = (elem_t)tot;  // parameter order [C][3][3]
  }
}

// --------------------------------------------------------------- host side

static bool dw_is_16(const at::Tensor& t) {
  return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf;
}

// logical NCHW with channels_last strides; size-1 dims may carry any stride
static bool dw_is_nhwc(const at::Tensor& t) {
  if (t.dim() != 4) return false;
  long C = t.size(1), H = t.size(2), W = t.size(3);
  long want[4] = {H * W * C, 1, W * C, C};
  for (int d = 0; d < 4; ++d)
    if (t.size(d) > 1 && t.stride(d) != want[d]) return false;
  return true;
}

static bool dw_aligned16(const at::Tensor& t) {
  return ((uintptr_t)t.data_ptr() & 15) == 0;
}

// the supported envelope, shared by the three entry points. `a` is the
// activation-shaped tensor that fixes dtype and C.
static void dw_check_act(const char* op, const char* name, const at::Tensor& a) {
  TORCH_CHECK(a.is_cuda() && dw_is_16(a), op, ": ", name,
              " must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(a.dim() == 4 && a.numel() > 0, op, ": ", name,
              " must be a non-empty 4-D (N,C,H,W) tensor");
  TORCH_CHECK(a.size(1) % 8 == 0, op, ": depthwise kernels need C % 8 == 0, got C=",
              a.size(1));
  TORCH_CHECK(dw_is_nhwc(a), op, ": ", name,
              " must be channels_last (NHWC) in memory");
  TORCH_CHECK(dw_aligned16(a), op, ": ", name, " must be 16-byte aligned");
  TORCH_CHECK(a.numel() < (1ll << 31), op, ": ", name, " too large (>= 2^31 elements)");
}

static void dw_check_sp(const char* op, long stride, long pad) {
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ", stride);
  TORCH_CHECK(pad == 0 || pad == 1, op, ": padding must be 0 or 1, got ", pad);
}

static void dw_check_w(const char* op, const at::Tensor& w, const at::Tensor& a) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == a.scalar_type() &&
                  w.device() == a.device(),
              op, ": weight must be on the same device and of the same dtype");
  TORCH_CHECK(w.dim() == 4 && w.size(1) == 1 && w.size(2) == 3 && w.size(3) == 3,
              op, ": depthwise kernels support 3x3 weights of shape (C,1,3,3) only");
  TORCH_CHECK(w.size(0) == a.size(1), op,
              ": weight has ", w.size(0), " channels, input has ", a.size(1));
  // contiguous and channels_last views of (C,1,3,3) share memory order [C][3][3]
  TORCH_CHECK(w.numel() == 9 * a.size(1) && w.stride(0) == 9 && w.stride(2) == 3 &&
                  w.stride(3) == 1,
              op, ": weight memory must be [C][3][3] (dense (C,1,3,3))");
  TORCH_CHECK(dw_aligned16(w), op, ": weight must be 16-byte aligned");
}

static bool dw_out_dims(long H, long W, long stride, long pad, long& P, long& Q) {
  if (H + 2 * pad < 3 || W + 2 * pad < 3) return false;
  P = (H + 2 * pad - 3) / stride + 1;
  Q = (W + 2 * pad - 3) / stride + 1;
  return true;
}

static uint32_t dw_grid(uint32_t total) {
  uint32_t b = (total + DW_THREADS - 1) / DW_THREADS;
  return b < (uint32_t)DW_MAX_BLOCKS ? b : (uint32_t)DW_MAX_BLOCKS;
}

at::Tensor dwconv_fwd(const at::Tensor& x, const at::Tensor& w, long stride,
                      long pad) {
  dw_check_act("dwconv_fwd", "x", x);
  dw_check_sp("dwconv_fwd", stride, pad);
  dw_check_w("dwconv_fwd", w, x);
  long N = x.size(0), C = x.size(1), H = x.size(2), W_ = x.size(3), P, Q;
  TORCH_CHECK(dw_out_dims(H, W_, stride, pad, P, Q),
              "dwconv_fwd: input smaller than the 3x3 window");
  auto y = at::empty({N, C, P, Q}, x.options(), at::MemoryFormat::ChannelsLast);
  uint32_t cvecs = C / 8, QS = (Q + DW_STRIP - 1) / DW_STRIP;
  uint32_t total = (uint32_t)(N * P) * QS * cvecs;
  FastDiv dCv, dQs, dP;
  dCv.init(cvecs);
  dQs.init(QS);
  dP.init((uint32_t)P);
  DTMX_DISPATCH_16(x.scalar_type(), "dwconv_fwd", {
    auto xp = (const elem_t*)x.data_ptr();
    auto wp = (const elem_t*)w.data_ptr();
    auto yp = (elem_t*)y.data_ptr();
    if (stride == 1)
      dwconv_fwd_kernel<elem_t, 1><<<dw_grid(total), DW_THREADS, 0, dw_stream()>>>(
          xp, wp, yp, C, H, W_, P, Q, (int)pad, total, dCv, dQs, dP);
    else
      dwconv_fwd_kernel<elem_t, 2><<<dw_grid(total), DW_THREADS, 0, dw_stream()>>>(
          xp, wp, yp, C, H, W_, P, Q, (int)pad, total, dCv, dQs, dP);
  });
  return y;
}

at::Tensor dwconv_dgrad(const at::Tensor& dy, const at::Tensor& w, long stride,
                        long pad, long H, long W_) {
  dw_check_act("dwconv_dgrad", "dy", dy);
  dw_check_sp("dwconv_dgrad", stride, pad);
  dw_check_w("dwconv_dgrad", w, dy);
  long N = dy.size(0), C = dy.size(1), P, Q;
  TORCH_CHECK(H > 0 && W_ > 0 && dw_out_dims(H, W_, stride, pad, P, Q) &&
                  P == dy.size(2) && Q == dy.size(3),
              "dwconv_dgrad: dy spatial size does not match H, W, stride, pad");
  TORCH_CHECK(N * C * H * W_ < (1ll << 31), "dwconv_dgrad: dx too large");
  auto dx = at::empty({N, C, H, W_}, dy.options(), at::MemoryFormat::ChannelsLast);
  uint32_t cvecs = C / 8, WS = (W_ + DW_STRIP - 1) / DW_STRIP;
  uint32_t total = (uint32_t)(N * H) * WS * cvecs;
  FastDiv dCv, dWs, dH;
  dCv.init(cvecs);
  dWs.init(WS);
  dH.init((uint32_t)H);
#define DTMX_DW_DGRAD(S_, P_)                                                    \
  dwconv_dgrad_kernel<elem_t, S_, P_><<<dw_grid(total), DW_THREADS, 0,           \
                                        dw_stream()>>>(                          \
      (const elem_t*)dy.data_ptr(), (const elem_t*)w.data_ptr(),                 \
      (elem_t*)dx.data_ptr(), C, H, W_, P, Q, total, dCv, dWs, dH)
  DTMX_DISPATCH_16(dy.scalar_type(), "dwconv_dgrad", {
    if (stride == 1 && pad == 0) DTMX_DW_DGRAD(1, 0);
    else if (stride == 1) DTMX_DW_DGRAD(1, 1);
    else if (pad == 0) DTMX_DW_DGRAD(2, 0);
    else DTMX_DW_DGRAD(2, 1);
  });
#undef DTMX_DW_DGRAD
  return dx;
}

at::Tensor dwconv_wgrad(const at::Tensor& x, const at::Tensor& dy, long stride,
                        long pad) {
  dw_check_act("dwconv_wgrad", "x", x);
  dw_check_act("dwconv_wgrad", "dy", dy);
  dw_check_sp("dwconv_wgrad", stride, pad);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.device() == x.device(),
              "dwconv_wgrad: x and dy must share dtype and device");
  long N = x.size(0), C = x.size(1), H = x.size(2), W_ = x.size(3), P, Q;
  TORCH_CHECK(dw_out_dims(H, W_, stride, pad, P, Q) && dy.size(0) == N &&
                  dy.size(1) == C && dy.size(2) == P && dy.size(3) == Q,
              "dwconv_wgrad: dy shape does not match x, stride, pad");
  uint32_t cvecs = C / 8, QS = (Q + DW_STRIP - 1) / DW_STRIP;
  uint32_t nstrips = (uint32_t)(N * P) * QS;
  uint32_t cvb = cvecs < (uint32_t)DW_WG_CVB ? cvecs : (uint32_t)DW_WG_CVB;
  uint32_t groups = (cvecs + cvb - 1) / cvb;
  uint32_t PL = DW_THREADS / cvb;
  // enough blocks to fill the machine, but each lane keeps >= 4 strips so the
  // LDS fold and the partial round trip stay small next to the streaming
  uint32_t NB = (nstrips + PL * 4 - 1) / (PL * 4);
  uint32_t cap = DW_WG_BLOCKS / groups;
  if (NB > cap) NB = cap;
  if (NB < 1) NB = 1;
  auto part = at::empty({(long)NB, 9, C}, x.options().dtype(at::kFloat));
  auto dw = at::empty({C, 1, 3, 3}, x.options());
  FastDiv dQs, dP;
  dQs.init(QS);
  dP.init((uint32_t)P);
  DTMX_DISPATCH_16(x.scalar_type(), "dwconv_wgrad", {
    auto xp = (const elem_t*)x.data_ptr();
    auto gp = (const elem_t*)dy.data_ptr();
    auto pp = part.data_ptr<float>();
    dim3 grid(NB, groups);
    if (stride == 1)
      dwconv_wgrad_partial_kernel<elem_t, 1><<<grid, DW_THREADS, 0, dw_stream()>>>(
          xp, gp, pp, C, H, W_, P, Q, (int)pad, nstrips, cvb, PL, dQs, dP);
    else
      dwconv_wgrad_partial_kernel<elem_t, 2><<<grid, DW_THREADS, 0, dw_stream()>>>(
          xp, gp, pp, C, H, W_, P, Q, (int)pad, nstrips, cvb, PL, dQs, dP);
    uint32_t fb = (9 * (uint32_t)C + DW_FIN_I - 1) / DW_FIN_I;
    dwconv_wgrad_finalize_kernel<elem_t><<<fb, DW_THREADS, 0, dw_stream()>>>(
        pp, (elem_t*)dw.data_ptr(), C, NB);
  });
  return dw;
}

}  // namespace dtmx
