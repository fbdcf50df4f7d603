// Line convolution (1xT / Tx1, fwd and dgrad) for gfx950, NHWC.
// (reference src/operator/nn/convolution.cu with kernel=(1,7) pad=(0,3) and
// its transposes — the factorised towers of Inception-v3/v4/ResNet-v2.)
//
// Stride 1, dilation 1, padding (T-1)/2 on the tap axis only: input and
// output share the flattened pixel index m = (n,h,w), and output row m reads
// input rows m + (t - pad) d with d = 1 (1xT) or d = W (Tx1). The im2col
// matrix is therefore the activation itself read with overlapping rows:
//
//   out[m][n] = sum_t sum_k  A[m + (t - pad) d][k] . B[n][t][k]
//
//   fwd    A = x  [M][C],  B = w  [Ko][T][C]   (the parameter as stored)
//   dgrad  A = dy [M][Ko], B = wp [C][T'][Ko]  (packed per call, T' = T-1-t:
//          the taps reversed, each tap's weight transposed)
//
// One block owns 128 consecutive pixels and a 128-wide slice of the output
// channels. Per chunk of 64 contraction channels it stages the window
// [128 + (T-1) d rows][64 ch] ONCE (global_load_lds, double-buffered) and
// streams the T weight tiles [128][64] through a two-slot ring; tap t runs
// v_mfma_f32_16x16x32 off window rows shifted by t d. The generic gather
// kernel stages the same pixels T times and pays two FastDiv decodes per
// 16-byte piece; here staging is division-free.
//
// Swizzle: piece p of window row r is stored at p ^ ((r >> 1) & 7), applied
// on the glds source side. A fragment reads 16 consecutive rows; (r & 1, piece)
// then takes 16 distinct values for ANY 16 consecutive rows, so the read is
// conflict-free under every tap shift t d, not only at multiples of 8 rows.
//
// Border: a tap whose coordinate on the tap axis leaves the image contributes
// zero. The same window row is valid for one output and invalid for its
// neighbour, so it cannot be staged as zeros: each lane computes a T-bit mask
// per fragment row once per tile and clears the A fragment in registers. The
// mask also keeps image n from reading n +- 1 and (1xT) row h from h +- 1.
//
// fp32 accumulation, LDS-staged 16-byte stores, every output element written
// exactly once: no atomics, no zero fill, bit-identical run to run.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"
#include "lineconv.h"

namespace dtmx {

static hipStream_t lc_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int LC_THREADS = 256;                 // 4 waves, 2 x 2, 64 x 64 each
constexpr int LC_BM = 128, LC_BN = 128, LC_BK = 64;
constexpr int LC_ROWB = LC_BK * 2;              // bytes of one LDS row
constexpr int LC_GRP = LC_THREADS * 16 / LC_ROWB;  // rows per glds round: 32
constexpr int LC_GRP_B = LC_GRP * LC_ROWB;      // 4 KiB
constexpr int LC_NJ = LC_BN / LC_GRP;           // glds rounds per weight tile
constexpr int LC_TILE_B = LC_BN * LC_ROWB;      // 16 KiB
constexpr int LC_MAX_HALO = 256;                // (T-1) d, window rows

__device__ __forceinline__ uint32_t lc_swz(uint32_t row) { return (row >> 1) & 7; }

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the window's glds count
// depends on W). Waiting for fewer loads in flight than asked is always safe.
__device__ __forceinline__ void lc_wait_vmcnt(uint32_t n) {
#define DTMX_LC_W(N_) \
  case N_: asm volatile("s_waitcnt vmcnt(" #N_ ")" ::: "memory"); break;
  switch (n) {
    DTMX_LC_W(1) DTMX_LC_W(2) DTMX_LC_W(3) DTMX_LC_W(4) DTMX_LC_W(5) DTMX_LC_W(6)
    DTMX_LC_W(7) DTMX_LC_W(8) DTMX_LC_W(9) DTMX_LC_W(10) DTMX_LC_W(11)
    DTMX_LC_W(12) DTMX_LC_W(13) DTMX_LC_W(14) DTMX_LC_W(15) DTMX_LC_W(16)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef DTMX_LC_W
}

// ----------------------------------------------------------- dgrad weight pack

// wp[c][T-1-t][ko] = w[ko][t][c]; thread i = (ko8, t, c), c fastest, writes the
// eight ko of one 16-byte piece.
template <typename elem_t>
__global__ __launch_bounds__(LC_THREADS) void lineconv_pack_kernel(
    const elem_t* __restrict__ w, elem_t* __restrict__ wp, uint32_t total,
    uint32_t C, uint32_t Ko, uint32_t T) {
  using V8 = typename E8<elem_t>::v8;
  uint32_t i = blockIdx.x * LC_THREADS + threadIdx.x;
  if (i >= total) return;
  uint32_t c = i % C, r = i / C;
  uint32_t t = r % T, ko8 = r / T;
  V8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w[((size_t)(ko8 * 8 + j) * T + t) * C + c];
  *(V8*)(wp + ((size_t)c * T + (T - 1 - t)) * Ko + ko8 * 8) = v;
}

// ------------------------------------------------------------------- kernel

// WRG = 32-row glds rounds the window buffer holds (5: 1xT and short halos,
// 8 / 12: Tx1 halos up to 128 / 256 rows). LDS = 2 windows + 2 weight tiles:
// 72 / 96 / 128 KiB, so two blocks share a CU only at WRG = 5.
//
// Load order, which the counted waits rely on (vmcnt retires in order):
//   prologue      win 0, tile 0, tile 1, win 1
//   end of step s tile s + 2, then win c + 2 if s is the last step of chunk c
// so at the top of step s = c T + t everything issued after tile s is tile
// s + 1, plus window c + 1 when t < 2.
template <typename elem_t, int T, int WRG>
__global__ __launch_bounds__(LC_THREADS, WRG == 5 ? 2 : 1) void lineconv_kernel(
    const elem_t* __restrict__ a, const elem_t* __restrict__ b,
    elem_t* __restrict__ out, const elem_t* __restrict__ zero, uint32_t M,
    uint32_t K, uint32_t Nn, uint32_t ldb, uint32_t d, uint32_t L,
    uint32_t vertical, FastDiv dW, FastDiv dH, uint32_t tiles_n) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int PAD = (T - 1) / 2;
  constexpr uint32_t WIN_B = WRG * LC_GRP_B;
  static_assert(2 * WIN_B >= LC_BM * LC_BN * 2, "the C tile reuses the windows");
  __shared__ __attribute__((aligned(16))) char smem[2 * WIN_B + 2 * LC_TILE_B];
  char* const win = smem;
  char* const ring = smem + 2 * WIN_B;

  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const uint32_t bm = (bid / tiles_n) * LC_BM, bn = (bid % tiles_n) * LC_BN;
  const uint32_t nch = (K + LC_BK - 1) / LC_BK, nsteps = nch * T;
  const uint32_t wrows = LC_BM + (T - 1) * d;            // window rows in use
  const uint32_t wgr = (wrows + LC_GRP - 1) / LC_GRP;    // glds rounds, <= WRG

  // staging slot: round `it` covers LDS row it * 32 + srow, piece tid & 7;
  // 32 | the round stride, so one swizzle term serves every round
  const uint32_t srow = tid >> 3;
  const uint32_t sk = ((tid & 7) ^ lc_swz(srow)) << 3;   // source channel offset
  const int64_t m0 = (int64_t)bm - (int64_t)PAD * d + srow;  // pixel of row srow

  auto stage_win = [&](uint32_t buf, uint32_t c) {
    const uint32_t k = c * LC_BK + sk;
    for (uint32_t it = 0; it < wgr; ++it) {
      const int64_t m = m0 + it * LC_GRP;
      const bool ok = m >= 0 && m < (int64_t)M && k < K &&
                      it * LC_GRP + srow < wrows;
      glds16(ok ? a + (size_t)m * K + k : zero,
             win + buf * WIN_B + it * LC_GRP_B + wave * 1024);
    }
  };
  const elem_t* brow[LC_NJ];
#pragma unroll
  for (int it = 0; it < LC_NJ; ++it) {
    const uint32_t n = bn + it * LC_GRP + srow;
    brow[it] = n < Nn ? b + (size_t)n * ldb : nullptr;
  }
  auto stage_tile = [&](uint32_t slot, uint32_t c, uint32_t t) {
    const uint32_t k = c * LC_BK + sk;
#pragma unroll
    for (int it = 0; it < LC_NJ; ++it)
      glds16(brow[it] && k < K ? brow[it] + (size_t)t * K + k : zero,
             ring + slot * LC_TILE_B + it * LC_GRP_B + wave * 1024);
  };

  // tap validity of this lane's four fragment rows: bit t of msk[i]
  const uint32_t wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  uint32_t msk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = bm + wr + i * 16 + (lane & 15);
    msk[i] = 0;
    if (m < M) {
      const uint32_t q = dW.div(m);
      const uint32_t pos = vertical ? dH.mod(q, dH.div(q)) : dW.mod(m, q);
#pragma unroll
      for (int t = 0; t < T; ++t)
        msk[i] |= (uint32_t)(pos + t - PAD < L) << t;  // unsigned: < 0 wraps high
    }
  }

  f32x4 acc[4][4] = {};
  stage_win(0, 0);
  stage_tile(0, 0, 0);
  stage_tile(1, 0, 1);
  if (nch > 1) stage_win(1, 1);
  for (uint32_t c = 0; c < nch; ++c) {
    const char* wbuf = win + (c & 1) * WIN_B;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint32_t s = c * T + t;
      lc_wait_vmcnt((s + 1 < nsteps ? LC_NJ : 0) +
                    (t < 2 && c + 1 < nch ? wgr : 0));
      __builtin_amdgcn_s_barrier();
      const char* tb = ring + (s & 1) * LC_TILE_B;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        V8 af[4], bfr[4];
        const uint32_t p = kk * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t row = wr + i * 16 + (lane & 15) + t * d;  // window row
          V8 v = *(const V8*)(wbuf + row * LC_ROWB + ((p ^ lc_swz(row)) << 4));
          V8 z = {};
          af[i] = (msk[i] >> t) & 1 ? v : z;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t row = wc + j * 16 + (lane & 15);
          bfr[j] = *(const V8*)(tb + row * LC_ROWB + ((p ^ lc_swz(row)) << 4));
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = E8<elem_t>::mfma(af[i], bfr[j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
      __builtin_amdgcn_s_barrier();  // every wave done with slot s & 1
      if (s + 2 < nsteps) stage_tile(s & 1, c + (t + 2) / T, (t + 2) % T);
      if (t == T - 1 && c + 2 < nch) stage_win(c & 1, c + 2);
    }
  }

  // C tile through LDS: 16-byte row chunks with M and N tails (N % 8 == 0).
  // Nothing is in flight: the last step waited for vmcnt(0).
  __syncthreads();
  elem_t* ct = (elem_t*)smem;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t col = wc + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wr + i * 16 + ((lane >> 4) << 2) + r) * LC_BN + col] =
            (elem_t)acc[i][j][r];
    }
  __syncthreads();
  for (uint32_t idx = tid; idx < LC_BM * LC_BN / 8; idx += LC_THREADS) {
    const uint32_t row = idx / (LC_BN / 8), nc = idx % (LC_BN / 8);
    const uint32_t m = bm + row, n = bn + nc * 8;
    if (m < M && n < Nn)
      *(V8*)(out + (size_t)m * Nn + n) = *(const V8*)(ct + row * LC_BN + nc * 8);
  }
}

// --------------------------------------------------------------- host side

// a zeroed 16-bit pattern reads as 0.0 in bf16 and fp16 alike
static const void* lc_zero_page(const at::Tensor& like) {
  static at::Tensor z;
  if (!z.defined() || z.device() != like.device())
    z = at::zeros({64}, like.options().dtype(at::kBFloat16));
  return z.data_ptr();
}

struct LcShape {
  long N, H, W, C, Ko, T;
  bool vertical;  // Tx1
};

// `a` is x (fwd) or dy (dgrad); both have the spatial size of the other
static LcShape lc_check(const char* op, const char* aname, const at::Tensor& a,
                        const at::Tensor& w, bool a_is_dy) {
  TORCH_CHECK(a.is_cuda() && (a.scalar_type() == at::kBFloat16 ||
                              a.scalar_type() == at::kHalf),
              op, ": ", aname, " must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == a.scalar_type() &&
                  w.device() == a.device(),
              op, ": w must be on the device of ", aname, " and of its dtype");
  TORCH_CHECK(a.dim() == 4 && a.numel() > 0 &&
                  a.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": ", aname, " must be a non-empty 4-D NHWC (channels_last) tensor");
  TORCH_CHECK(w.dim() == 4 && w.numel() > 0 &&
                  w.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": w must be a non-empty 4-D KRSC (channels_last) tensor");
  LcShape s;
  s.N = a.size(0); s.H = a.size(2); s.W = a.size(3);
  s.Ko = w.size(0); s.C = w.size(1);
  const long R = w.size(2), S = w.size(3);
  TORCH_CHECK((R == 1) != (S == 1), op, ": the kernel must be 1xT or Tx1, got ", R,
              "x", S);
  s.vertical = S == 1;
  s.T = s.vertical ? R : S;
  TORCH_CHECK(s.T == 3 || s.T == 5 || s.T == 7, op,
              ": T must be 3, 5 or 7, got ", s.T);
  TORCH_CHECK(s.C % 8 == 0, op, ": C % 8 == 0 required, got C = ", s.C);
  TORCH_CHECK(s.Ko % 8 == 0, op, ": Ko % 8 == 0 required, got Ko = ", s.Ko);
  TORCH_CHECK(a.size(1) == (a_is_dy ? s.Ko : s.C), op, ": ", aname, " has ",
              a.size(1), " channels, w wants ", a_is_dy ? s.Ko : s.C);
  // w rows are glds sources like the generic kernels' B operand: parameters
  // are views into flat optimizer buckets and carry element alignment only
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0, op, ": ", aname,
              " must be 16-byte aligned");
  TORCH_CHECK(s.N * s.H * s.W < (1ll << 31), op,
              ": N*H*W < 2^31 required, got ", s.N * s.H * s.W);
  TORCH_CHECK(w.numel() < (1ll << 31), op, ": w too large (>= 2^31 elements)");
  TORCH_CHECK(!s.vertical || (s.T - 1) * s.W <= LC_MAX_HALO, op,
              ": Tx1 needs a halo (T-1)*W of at most ", LC_MAX_HALO,
              " rows, got ", (s.T - 1) * s.W);
  return s;
}

// out[M][Nn] from A [M][K] and B [Nn][T][K]
template <typename elem_t>
static void lc_launch(const LcShape& s, const void* a, const void* b, void* out,
                      const void* zero, long K, long Nn) {
  const uint32_t M = (uint32_t)(s.N * s.H * s.W);
  const uint32_t d = s.vertical ? (uint32_t)s.W : 1u;
  const uint32_t L = (uint32_t)(s.vertical ? s.H : s.W);
  const uint32_t wrows = LC_BM + (uint32_t)(s.T - 1) * d;
  FastDiv dW, dH;
  dW.init((uint32_t)s.W);
  dH.init((uint32_t)s.H);
  const uint32_t tiles_m = (M + LC_BM - 1) / LC_BM;
  const uint32_t tiles_n = (uint32_t)((Nn + LC_BN - 1) / LC_BN);
#define DTMX_LC_RUN(T_, G_)                                                     \
  lineconv_kernel<elem_t, T_, G_>                                               \
      <<<tiles_m * tiles_n, LC_THREADS, 0, lc_stream()>>>(                      \
          (const elem_t*)a, (const elem_t*)b, (elem_t*)out, (const elem_t*)zero, \
          M, (uint32_t)K, (uint32_t)Nn, (uint32_t)(s.T * K), d, L,              \
          s.vertical ? 1u : 0u, dW, dH, tiles_n)
#define DTMX_LC_RUN_T(T_)                                   \
  do {                                                      \
    if (wrows <= 5 * LC_GRP) DTMX_LC_RUN(T_, 5);            \
    else if (wrows <= 8 * LC_GRP) DTMX_LC_RUN(T_, 8);       \
    else DTMX_LC_RUN(T_, 12);                               \
  } while (0)
  static_assert(LC_BM + LC_MAX_HALO <= 12 * LC_GRP, "largest window buffer");
  if (s.T == 3) DTMX_LC_RUN_T(3);
  else if (s.T == 5) DTMX_LC_RUN_T(5);
  else DTMX_LC_RUN_T(7);
#undef DTMX_LC_RUN_T
#undef DTMX_LC_RUN
}

void lineconv_pack(const at::Tensor& w, at::Tensor& wp, long C, long Ko, long T) {
  const uint32_t total = (uint32_t)(C * T * (Ko / 8));
  DTMX_DISPATCH_16(w.scalar_type(), "lineconv_pack", {
    lineconv_pack_kernel<elem_t>
        <<<(total + LC_THREADS - 1) / LC_THREADS, LC_THREADS, 0, lc_stream()>>>(
            (const elem_t*)w.data_ptr(), (elem_t*)wp.data_ptr(), total,
            (uint32_t)C, (uint32_t)Ko, (uint32_t)T);
  });
}

at::Tensor lineconv_fwd(const at::Tensor& x, const at::Tensor& w) {
  const LcShape s = lc_check("lineconv_fwd", "x", x, w, false);
  auto y = at::empty({s.N, s.Ko, s.H, s.W}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  const void* zero = lc_zero_page(x);
  DTMX_DISPATCH_16(x.scalar_type(), "lineconv_fwd", {
    lc_launch<elem_t>(s, x.data_ptr(), w.data_ptr(), y.data_ptr(), zero, s.C, s.Ko);
  });
  return y;
}

at::Tensor lineconv_dgrad(const at::Tensor& dy, const at::Tensor& w) {
  const LcShape s = lc_check("lineconv_dgrad", "dy", dy, w, true);
  auto dx = at::empty({s.N, s.C, s.H, s.W}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  auto wp = at::empty({s.C, s.T, s.Ko}, dy.options());
  const void* zero = lc_zero_page(dy);
  lineconv_pack(w, wp, s.C, s.Ko, s.T);
  DTMX_DISPATCH_16(dy.scalar_type(), "lineconv_dgrad", {
    lc_launch<elem_t>(s, dy.data_ptr(), wp.data_ptr(), dx.data_ptr(), zero, s.Ko,
                      s.C);
  });
  return dx;
}

}  // namespace dtmx
