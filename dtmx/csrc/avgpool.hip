// Windowed average pooling (fwd / bwd) for gfx950, NHWC.
// (reference src/operator/nn/pool.cuh pool_sum_2d / unpool_sum_2d with the
// avg divisor, both padding conventions — the pool branch every Inception
// unit opens with.)
//
// No weights, no saved state: a pure bandwidth op. One thread owns a
// bf16x8/f16x8 channel vector (16-B loads/stores, lanes walk C first so a
// wave reads whole NHWC rows); sums are fp32 with one convert at the store.
//
// Divisor of window (p, q), torch's semantics: the window [p*s - pad,
// p*s - pad + K) is clipped to the padded extent [-pad, H + pad); that count
// is the divisor with count_include_pad, the count of positions inside
// [0, H) is the divisor without. Both factor into a row count times a
// column count, so backward recomputes them from (p, q) and saves nothing.
//
// Two code paths per direction:
//   3x3 stride 1 pad 1 (the Inception case): the box filter is separable, so
//     a thread takes a strip of AP_STRIP outputs along W, loads the
//     AP_STRIP + 2 columns of each of the 3 rows once, keeps per-column
//     vertical sums and forms each output from three of them — 4.5 loads per
//     output, not 9. Backward is the same box over dy with the per-source
//     weight 1/div folded in (row factor while summing, column factor after,
//     both as exact small integers over a common 1/36).
//   every other (K, stride, pad) in the envelope: runtime loops, one thread
//     per output channel vector; backward in gather form (each dx element
//     sums the windows that contain it), so every dx element is written once
//     and there are no atomics and no zero fill.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"

namespace dtmx {

static hipStream_t ap_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int AP_THREADS = 256;
constexpr int AP_STRIP = 4;          // outputs per thread along W (3x3 s1 p1)
constexpr int AP_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; grid-stride the rest
constexpr int AP_MIN_K = 2, AP_MAX_K = 8, AP_MAX_STRIDE = 8;

template <typename elem_t>
__device__ __forceinline__ typename E8<elem_t>::v8 ap_zero() {
  typename E8<elem_t>::v8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (elem_t)0.f;
  return z;
}

// positions of [i, i + 3) inside [0, n), for i >= -1 and i + 3 <= n + 1
__device__ __forceinline__ int ap_count3(int i, int n) {
  return 3 - (i < 0) - (i + 3 > n);
}

// ---------------------------------------------------- 3x3 stride 1 pad 1

// work item = (n, p, q-strip, c8), c8 fastest. Padding by predication.
// Output size equals input size, and every window lies inside the padded
// extent, so the include-pad divisor is 9 everywhere.
template <typename elem_t, bool INCLUDE_PAD>
__global__ __launch_bounds__(AP_THREADS) void avgpool3_fwd_kernel(
    const elem_t* __restrict__ x, elem_t* __restrict__ y, uint32_t C,
    uint32_t H, uint32_t W, uint32_t total, FastDiv dCv, FastDiv dQs,
    FastDiv dP) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int S = AP_STRIP;
  const uint32_t step = gridDim.x * AP_THREADS;
  for (uint32_t i = blockIdx.x * AP_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dQs.div(m), qs = dQs.mod(m, r);
    uint32_t n = dP.div(r), p = dP.mod(r, n);
    float cs[S + 2][8];  // vertical sums of the strip's columns
#pragma unroll
    for (int c = 0; c < S + 2; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) cs[c][e] = 0.f;
    const int ih0 = (int)p - 1;
    const int iw0 = (int)(qs * S) - 1;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int ih = ih0 + kh;
      if ((uint32_t)ih >= H) continue;
      const elem_t* row = x + ((size_t)n * H + (uint32_t)ih) * W * C + cv * 8;
      V8 col[S + 2];
#pragma unroll
      for (int c = 0; c < S + 2; ++c) {
        int iw = iw0 + c;
        col[c] = (uint32_t)iw < W ? *(const V8*)(row + (size_t)(uint32_t)iw * C)
                                  : ap_zero<elem_t>();
      }
#pragma unroll
      for (int c = 0; c < S + 2; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) cs[c][e] += (float)col[c][e];
    }
    const int rows = ap_count3(ih0, (int)H);
    elem_t* out = y + (((size_t)n * H + p) * W + qs * S) * C + cv * 8;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (qs * S + j >= W) break;
      const float inv =
          INCLUDE_PAD ? 1.f / 9.f
                      : 1.f / (float)(rows * ap_count3(iw0 + j, (int)W));
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[e] = (elem_t)((cs[j][e] + cs[j + 1][e] + cs[j + 2][e]) * inv);
      *(V8*)(out + (size_t)j * C) = o;
    }
  }
}

// dx[n,h,w] = sum over the windows (p, q) in [h-1, h+1] x [w-1, w+1] inside
// dy of dy[n,p,q] / div(p, q) — a 3x3 box over dy with a per-source weight.
// div(p, q) = rows(p) * cols(q) with both counts in {1, 2, 3}, so
// 1/div = (6/rows) * (6/cols) / 36 with small-integer factors: 6/rows(p)
// scales dy row p as it is summed, 6/cols(q) scales column sum q, and one
// multiply by 1/36 (1/9 with include-pad) finishes each output. Integer
// weights keep every partial sum exact where the result is, which separate
// roundings of 1/3 and 1/9 per term would not under cancellation.
// work item = (n, h, w-strip, c8).
template <typename elem_t, bool INCLUDE_PAD>
__global__ __launch_bounds__(AP_THREADS) void avgpool3_bwd_kernel(
    const elem_t* __restrict__ dy, elem_t* __restrict__ dx, uint32_t C,
    uint32_t H, uint32_t W, uint32_t total, FastDiv dCv, FastDiv dWs,
    FastDiv dH) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int S = AP_STRIP;
  const uint32_t step = gridDim.x * AP_THREADS;
  for (uint32_t i = blockIdx.x * AP_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dWs.div(m), ws = dWs.mod(m, r);
    uint32_t n = dH.div(r), h = dH.mod(r, n);
    float cs[S + 2][8];
#pragma unroll
    for (int c = 0; c < S + 2; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) cs[c][e] = 0.f;
    const int p0 = (int)h - 1;
    const int q0 = (int)(ws * S) - 1;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int p = p0 + kh;
      if ((uint32_t)p >= H) continue;
      const elem_t* row = dy + ((size_t)n * H + (uint32_t)p) * W * C + cv * 8;
      V8 col[S + 2];
#pragma unroll
      for (int c = 0; c < S + 2; ++c) {
        int q = q0 + c;
        col[c] = (uint32_t)q < W ? *(const V8*)(row + (size_t)(uint32_t)q * C)
                                 : ap_zero<elem_t>();
      }
      // window p covers input rows [p-1, p+2)
      const float rw = INCLUDE_PAD ? 1.f : (float)(6 / ap_count3(p - 1, (int)H));
#pragma unroll
      for (int c = 0; c < S + 2; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          cs[c][e] += INCLUDE_PAD ? (float)col[c][e] : (float)col[c][e] * rw;
    }
    if (!INCLUDE_PAD) {
#pragma unroll
      for (int c = 0; c < S + 2; ++c) {
        // out-of-range columns hold zeros and their count is still >= 1
        const float cw = (float)(6 / ap_count3(q0 + c - 1, (int)W));
#pragma unroll
        for (int e = 0; e < 8; ++e) cs[c][e] *= cw;
      }
    }
    elem_t* out = dx + (((size_t)n * H + h) * W + ws * S) * C + cv * 8;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (ws * S + j >= W) break;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = cs[j][e] + cs[j + 1][e] + cs[j + 2][e];
        o[e] = (elem_t)(v * (INCLUDE_PAD ? 1.f / 9.f : 1.f / 36.f));
      }
      *(V8*)(out + (size_t)j * C) = o;
    }
  }
}

// ------------------------------------------------------------ generic path

// [lo, hi) = window o along one axis of length n, clipped to the image;
// returns the divisor factor of that axis.
__device__ __forceinline__ int ap_span(int o, int n, int K, int u, int pad,
                                       bool include_pad, int& lo, int& hi) {
  int s = o * u - pad;
  int e = min(s + K, n + pad);
  int padded = e - s;
  lo = max(s, 0);
  hi = min(e, n);
  return include_pad ? padded : hi - lo;
}

// one thread = one output channel vector; work item = (n, p, q, c8)
template <typename elem_t>
__global__ __launch_bounds__(AP_THREADS) void avgpool_fwd_kernel(
    const elem_t* __restrict__ x, elem_t* __restrict__ y, uint32_t C,
    uint32_t H, uint32_t W, int K, int u, int pad, bool include_pad,
    uint32_t total, FastDiv dCv, FastDiv dQ, FastDiv dP) {
  using V8 = typename E8<elem_t>::v8;
  const uint32_t step = gridDim.x * AP_THREADS;
  for (uint32_t i = blockIdx.x * AP_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dQ.div(m), q = dQ.mod(m, r);
    uint32_t n = dP.div(r), p = dP.mod(r, n);
    int h0, h1, w0, w1;
    int div = ap_span((int)p, (int)H, K, u, pad, include_pad, h0, h1) *
              ap_span((int)q, (int)W, K, u, pad, include_pad, w0, w1);
    float acc[8] = {};
    for (int ih = h0; ih < h1; ++ih) {
      const elem_t* row = x + ((size_t)n * H + (uint32_t)ih) * W * C + cv * 8;
      for (int iw = w0; iw < w1; ++iw) {
        V8 v = *(const V8*)(row + (size_t)(uint32_t)iw * C);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
      }
    }
    const float fdiv = (float)div;
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (elem_t)(acc[e] / fdiv);
    *(V8*)(y + (size_t)m * C + cv * 8) = o;
  }
}

// gather form; work item = (n, h, w, c8). Elements no window reaches (far
// rows / columns at pad 0 with stride > 1) get an empty loop and store 0.
template <typename elem_t>
__global__ __launch_bounds__(AP_THREADS) void avgpool_bwd_kernel(
    const elem_t* __restrict__ dy, elem_t* __restrict__ dx, uint32_t C,
    uint32_t H, uint32_t W, uint32_t P, uint32_t Q, int K, int u, int pad,
    bool include_pad, uint32_t total, FastDiv dCv, FastDiv dW, FastDiv dH) {
  using V8 = typename E8<elem_t>::v8;
  const uint32_t step = gridDim.x * AP_THREADS;
  for (uint32_t i = blockIdx.x * AP_THREADS + threadIdx.x; i < total; i += step) {
    uint32_t m = dCv.div(i), cv = dCv.mod(i, m);
    uint32_t r = dW.div(m), w = dW.mod(m, r);
    uint32_t n = dH.div(r), h = dH.mod(r, n);
    // windows (p, q) that contain (h, w): p*u - pad <= h < p*u - pad + K
    int t = (int)h + pad - K + 1;
    int plo = t > 0 ? (t + u - 1) / u : 0;
    int phi = min(((int)h + pad) / u, (int)P - 1);
    t = (int)w + pad - K + 1;
    int qlo = t > 0 ? (t + u - 1) / u : 0;
    int qhi = min(((int)w + pad) / u, (int)Q - 1);
    float acc[8] = {};
    for (int p = plo; p <= phi; ++p) {
      int lo, hi;
      int dh = ap_span(p, (int)H, K, u, pad, include_pad, lo, hi);
      const elem_t* row = dy + ((size_t)n * P + (uint32_t)p) * Q * C + cv * 8;
      for (int q = qlo; q <= qhi; ++q) {
        const float fdiv =
            (float)(dh * ap_span(q, (int)W, K, u, pad, include_pad, lo, hi));
        V8 g = *(const V8*)(row + (size_t)(uint32_t)q * C);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)g[e] / fdiv;
      }
    }
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (elem_t)acc[e];
    *(V8*)(dx + (size_t)m * C + cv * 8) = o;
  }
}

// --------------------------------------------------------------- host side

// logical NCHW with channels_last strides; size-1 dims may carry any stride
static bool ap_is_nhwc(const at::Tensor& t) {
  long C = t.size(1), H = t.size(2), W = t.size(3);
  long want[4] = {H * W * C, 1, W * C, C};
  for (int d = 0; d < 4; ++d)
    if (t.size(d) > 1 && t.stride(d) != want[d]) return false;
  return true;
}

// the supported envelope, shared by both entry points
static void ap_check_act(const char* op, const char* name, const at::Tensor& a) {
  TORCH_CHECK(a.is_cuda() && (a.scalar_type() == at::kBFloat16 ||
                              a.scalar_type() == at::kHalf),
              op, ": ", name, " must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(a.dim() == 4 && a.numel() > 0, op, ": ", name,
              " must be a non-empty 4-D (N,C,H,W) tensor");
  TORCH_CHECK(a.size(1) % 8 == 0, op, ": avgpool kernels need C % 8 == 0, got C=",
              a.size(1));
  TORCH_CHECK(ap_is_nhwc(a), op, ": ", name,
              " must be channels_last (NHWC) in memory");
  TORCH_CHECK(((uintptr_t)a.data_ptr() & 15) == 0, op, ": ", name,
              " must be 16-byte aligned");
  TORCH_CHECK(a.numel() < (1ll << 31), op, ": ", name, " too large (>= 2^31 elements)");
}

static void ap_check_ksp(const char* op, long K, long stride, long pad) {
  TORCH_CHECK(K >= AP_MIN_K && K <= AP_MAX_K, op, ": kernel must be in [", AP_MIN_K,
              ", ", AP_MAX_K, "], got ", K);
  TORCH_CHECK(stride >= 1 && stride <= AP_MAX_STRIDE, op, ": stride must be in [1, ",
              AP_MAX_STRIDE, "], got ", stride);
  TORCH_CHECK(pad >= 0 && pad <= K / 2, op,
              ": padding must be in [0, kernel / 2], got ", pad, " for kernel ", K);
}

// floor mode
static bool ap_out_dims(long H, long W, long K, long stride, long pad, long& P,
                        long& Q) {
  if (H + 2 * pad < K || W + 2 * pad < K) return false;
  P = (H + 2 * pad - K) / stride + 1;
  Q = (W + 2 * pad - K) / stride + 1;
  return true;
}

static uint32_t ap_grid(uint32_t total) {
  uint32_t b = (total + AP_THREADS - 1) / AP_THREADS;
  return b < (uint32_t)AP_MAX_BLOCKS ? b : (uint32_t)AP_MAX_BLOCKS;
}

at::Tensor avgpool_fwd(const at::Tensor& x, long kernel, long stride, long pad,
                       bool count_include_pad) {
  ap_check_act("avgpool_fwd", "x", x);
  ap_check_ksp("avgpool_fwd", kernel, stride, pad);
  long N = x.size(0), C = x.size(1), H = x.size(2), W_ = x.size(3), P, Q;
  TORCH_CHECK(ap_out_dims(H, W_, kernel, stride, pad, P, Q),
              "avgpool_fwd: padded input smaller than the window (empty output)");
  auto y = at::empty({N, C, P, Q}, x.options(), at::MemoryFormat::ChannelsLast);
  const uint32_t cvecs = C / 8;
  const bool hot = kernel == 3 && stride == 1 && pad == 1;
  const uint32_t QS = hot ? (Q + AP_STRIP - 1) / AP_STRIP : (uint32_t)Q;
  const uint32_t total = (uint32_t)(N * P) * QS * cvecs;  // <= y.numel() / 8
  FastDiv dCv, dQ, dP;
  dCv.init(cvecs);
  dQ.init(QS);
  dP.init((uint32_t)P);
  DTMX_DISPATCH_16(x.scalar_type(), "avgpool_fwd", {
    auto xp = (const elem_t*)x.data_ptr();
    auto yp = (elem_t*)y.data_ptr();
    if (hot && count_include_pad)
      avgpool3_fwd_kernel<elem_t, true><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          xp, yp, C, H, W_, total, dCv, dQ, dP);
    else if (hot)
      avgpool3_fwd_kernel<elem_t, false><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          xp, yp, C, H, W_, total, dCv, dQ, dP);
    else
      avgpool_fwd_kernel<elem_t><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          xp, yp, C, H, W_, (int)kernel, (int)stride, (int)pad, count_include_pad,
          total, dCv, dQ, dP);
  });
  return y;
}

at::Tensor avgpool_bwd(const at::Tensor& dy, long H, long W_, long kernel,
                       long stride, long pad, bool count_include_pad) {
  ap_check_act("avgpool_bwd", "dy", dy);
  ap_check_ksp("avgpool_bwd", kernel, stride, pad);
  long N = dy.size(0), C = dy.size(1), P, Q;
  TORCH_CHECK(H > 0 && W_ > 0 && ap_out_dims(H, W_, kernel, stride, pad, P, Q) &&
                  P == dy.size(2) && Q == dy.size(3),
              "avgpool_bwd: dy spatial size does not match H, W, kernel, stride, pad");
  TORCH_CHECK(N * C * H * W_ < (1ll << 31), "avgpool_bwd: dx too large (>= 2^31 elements)");
  auto dx = at::empty({N, C, H, W_}, dy.options(), at::MemoryFormat::ChannelsLast);
  const uint32_t cvecs = C / 8;
  const bool hot = kernel == 3 && stride == 1 && pad == 1;
  const uint32_t WS = hot ? (W_ + AP_STRIP - 1) / AP_STRIP : (uint32_t)W_;
  const uint32_t total = (uint32_t)(N * H) * WS * cvecs;  // <= dx.numel() / 8
  FastDiv dCv, dW, dH;
  dCv.init(cvecs);
  dW.init(WS);
  dH.init((uint32_t)H);
  DTMX_DISPATCH_16(dy.scalar_type(), "avgpool_bwd", {
    auto gp = (const elem_t*)dy.data_ptr();
    auto dp = (elem_t*)dx.data_ptr();
    if (hot && count_include_pad)
      avgpool3_bwd_kernel<elem_t, true><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          gp, dp, C, H, W_, total, dCv, dW, dH);
    else if (hot)
      avgpool3_bwd_kernel<elem_t, false><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          gp, dp, C, H, W_, total, dCv, dW, dH);
    else
      avgpool_bwd_kernel<elem_t><<<ap_grid(total), AP_THREADS, 0, ap_stream()>>>(
          gp, dp, C, H, W_, (uint32_t)P, (uint32_t)Q, (int)kernel, (int)stride,
          (int)pad, count_include_pad, total, dCv, dW, dH);
  });
  return dx;
}

}  // namespace dtmx
