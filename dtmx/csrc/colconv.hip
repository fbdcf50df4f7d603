// Column convolution (Tx1, fwd and dgrad) for gfx950, NHWC.
// (reference src/operator/nn/convolution.cu with kernel=(7,1) pad=(3,0) — the
// vertical half of the factorised towers of Inception-v3/v4/ResNet-v2.)
//
//   y[n][h][w][ko] = sum_t sum_c  x[n][h + t - pad][w][c] . B[ko][t][c]
//
//   fwd    A = x,  B = w  [Ko][T][C]   (the parameter as stored)
//   dgrad  A = dy, B = wp [C][T'][Ko]  (lineconv_pack, per call: taps reversed,
//          each tap's weight transposed)
//
// A Tx1 convolution never mixes image columns, so the halo lies on H only.
// lineconv.hip runs Tx1 as a 1xT over the flattened pixel index with tap
// distance W and drags (T-1) W halo rows per 128-pixel tile; here a block owns
// whole columns and the halo is (T-1) image rows whatever W is.
//
// Strips: the columns of the whole batch are flattened, j = n W + w. A block
// owns CB = 8 consecutive j (they may straddle two images: columns never
// interact), a band of HB image rows and 128 output channels. Per chunk of 64
// contraction channels it stages the window [(HB + T - 1)][8][64 ch] ONCE
// (global_load_lds, double-buffered) and streams the T weight tiles [128][64]
// through a two-slot ring. Window row r = hh * 8 + jj holds image row
// h0 - pad + hh of column j0 + jj; rows outside [0, H) and columns >= N W are
// staged from the zero page, so the border costs nothing in the main loop.
//
// Taps are pure shifts: an output fragment is 16 consecutive window rows (two
// image rows by eight columns) and tap t reads the same fragment 8 t rows
// further down. No mask, no division in the loop; every LDS address is a
// per-lane base plus an immediate. Piece p of window row r is stored at
// p ^ ((r >> 1) & 7) (lineconv.hip's swizzle, applied on the glds source):
// (r & 1, piece) takes 16 distinct values over any 16 consecutive rows, so the
// fragment read is conflict-free under every shift.
//
// The four waves split the 128 output channels, 32 each, and every wave runs
// all MF fragments of the band (9 at H = 17, T = 7): the tile's height follows
// the image, 8 HB x 128. Fragments past the band (and the second image row of
// the last fragment of an odd band) compute on rows no output owns; the window
// buffer is sized for that over-read and the rows are not stored.
//
// fp32 accumulation, LDS-staged 16-byte stores, every output element written
// exactly once: no atomics, no zero fill, bit-identical run to run.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"
#include "lineconv.h"

namespace dtmx {

static hipStream_t cc_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int CC_THREADS = 256;                 // 4 waves, 1 x 4, MF*16 x 32 each
constexpr int CC_CB = 8;                        // columns of a strip
constexpr int CC_BN = 128, CC_BK = 64;
constexpr int CC_ROWB = CC_BK * 2;              // bytes of one LDS row
constexpr int CC_GRP = CC_THREADS * 16 / CC_ROWB;  // rows per glds round: 32
constexpr int CC_GRP_H = CC_GRP / CC_CB;        // image rows per glds round: 4
constexpr int CC_GRP_B = CC_GRP * CC_ROWB;      // 4 KiB
constexpr int CC_NJ = CC_BN / CC_GRP;           // glds rounds per weight tile
constexpr int CC_TILE_B = CC_BN * CC_ROWB;      // 16 KiB
constexpr int CC_MAX_WRG = 6;                   // largest window class

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the window's glds count
// depends on the band). Waiting for fewer loads in flight than asked is safe.
__device__ __forceinline__ void cc_wait_vmcnt(uint32_t n) {
#define DTMX_CC_W(N_) \
  case N_: asm volatile("s_waitcnt vmcnt(" #N_ ")" ::: "memory"); break;
  switch (n) {
    DTMX_CC_W(1) DTMX_CC_W(2) DTMX_CC_W(3) DTMX_CC_W(4) DTMX_CC_W(5) DTMX_CC_W(6)
    DTMX_CC_W(7) DTMX_CC_W(8) DTMX_CC_W(9) DTMX_CC_W(10)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef DTMX_CC_W
}
static_assert(CC_NJ + CC_MAX_WRG <= 10, "cc_wait_vmcnt covers tile + window");

// WRG = 32-row glds rounds the window buffer holds: 3 / 4 / 6 for windows of
// up to 12 / 16 / 24 image rows. LDS = 2 windows + 2 weight tiles, 56 / 64 /
// 80 KiB: two blocks share a CU in every class. MF = fragments of the tallest
// band of the class, 2 MF + T - 1 = 4 WRG image rows.
//
// Load order, which the counted waits rely on (vmcnt retires in order):
//   prologue      win 0, tile 0, tile 1, win 1
//   end of step s tile s + 2, then win c + 2 if s is the last step of chunk c
// so at the top of step s = c T + t everything issued after tile s is tile
// s + 1, plus window c + 1 when t < 2. Every thread issues the same count:
// masked rows load the zero page.
template <typename elem_t, int T, int WRG>
__global__ __launch_bounds__(CC_THREADS, 2) void colconv_kernel(
    const elem_t* __restrict__ a, const elem_t* __restrict__ b,
    elem_t* __restrict__ out, const elem_t* __restrict__ zero, uint32_t NW,
    uint32_t H, uint32_t W, uint32_t K, uint32_t Nn, uint32_t ldb, FastDiv dW,
    uint32_t tiles_n, uint32_t bands, uint32_t hb_base, uint32_t hb_rem) {
  using V8 = typename E8<elem_t>::v8;
  constexpr int PAD = (T - 1) / 2;
  constexpr int MF = (WRG * CC_GRP_H - (T - 1)) / 2;
  constexpr uint32_t WIN_B = WRG * CC_GRP_B;
  static_assert(MF * 16 + (T - 1) * CC_CB <= WRG * CC_GRP,
                "the last fragment's highest tap stays inside the window");
  static_assert(2 * WIN_B >= MF * 16 * CC_BN * 2, "the C tile reuses the windows");
  __shared__ __attribute__((aligned(16))) char smem[2 * WIN_B + 2 * CC_TILE_B];
  char* const win = smem;
  char* const ring = smem + 2 * WIN_B;

  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x);
  const uint32_t bn = (q % tiles_n) * CC_BN;
  q /= tiles_n;
  const uint32_t band = q % bands, j0 = (q / bands) * CC_CB;
  const uint32_t hb = hb_base + (band < hb_rem ? 1u : 0u);   // rows of the band
  const uint32_t h0 = band * hb_base + (band < hb_rem ? band : hb_rem);
  const uint32_t wimg = hb + T - 1;                          // window image rows
  const uint32_t wgr = (wimg + CC_GRP_H - 1) / CC_GRP_H;     // glds rounds, <= WRG
  const uint32_t nf = (hb + 1) / 2;                          // live fragments
  const uint32_t nch = (K + CC_BK - 1) / CC_BK, nsteps = nch * T;

  // staging slot: round `it` covers LDS row it * 32 + srow, piece tid & 7, so
  // a thread stages one column jj of four image rows apart; 32 | the round
  // stride, so one swizzle term and one (n, w) decode serve every round
  const uint32_t srow = tid >> 3;
  const uint32_t sk = ((tid & 7) ^ ((srow >> 1) & 7)) << 3;  // source channel
  const uint32_t sj = j0 + (srow & 7), shq = srow >> 3;
  const uint32_t sn = dW.div(sj);
  const size_t rowK = (size_t)W * K;
  const elem_t* const acol =                                 // pixel (n, 0, w)
      a + ((size_t)sn * H * W + dW.mod(sj, sn)) * K;

  auto stage_win = [&](uint32_t buf, uint32_t c) {
    const uint32_t k = c * CC_BK + sk;
    for (uint32_t it = 0; it < wgr; ++it) {
      const uint32_t hh = it * CC_GRP_H + shq;
      const uint32_t h = h0 + hh - PAD;                      // unsigned: < 0 wraps high
      const bool ok = sj < NW && hh < wimg && h < H && k < K;
      glds16(ok ? acol + (size_t)h * rowK + k : zero,
             win + buf * WIN_B + it * CC_GRP_B + wave * 1024);
    }
  };
  const elem_t* brow[CC_NJ];
#pragma unroll
  for (int it = 0; it < CC_NJ; ++it) {
    const uint32_t n = bn + it * CC_GRP + srow;
    brow[it] = n < Nn ? b + (size_t)n * ldb : nullptr;
  }
  auto stage_tile = [&](uint32_t slot, uint32_t c, uint32_t t) {
    const uint32_t k = c * CC_BK + sk;
#pragma unroll
    for (int it = 0; it < CC_NJ; ++it)
      glds16(brow[it] && k < K ? brow[it] + (size_t)t * K + k : zero,
             ring + slot * CC_TILE_B + it * CC_GRP_B + wave * 1024);
  };

  // fragment read offsets. Fragment i under tap t starts at window row
  // 16 i + 8 t, so its swizzle term is (l15 >> 1) ^ 4 (t & 1): two per-lane
  // bases per k half, everything else is an immediate
  const uint32_t l15 = lane & 15, wc = wave * 32;
  uint32_t aoff[2][2], boff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const uint32_t p = kk * 4 + (lane >> 4);
#pragma unroll
    for (int par = 0; par < 2; ++par)
      aoff[par][kk] = l15 * CC_ROWB + ((p ^ (l15 >> 1) ^ (par * 4)) << 4);
    boff[kk] = (wc + l15) * CC_ROWB + ((p ^ (l15 >> 1)) << 4);
  }

  f32x4 acc[MF][2] = {};
  stage_win(0, 0);
  stage_tile(0, 0, 0);
  stage_tile(1, 0, 1);
  if (nch > 1) stage_win(1, 1);
  for (uint32_t c = 0; c < nch; ++c) {
    const char* wbuf = win + (c & 1) * WIN_B;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint32_t s = c * T + t;
      cc_wait_vmcnt((s + 1 < nsteps ? CC_NJ : 0) +
                    (t < 2 && c + 1 < nch ? wgr : 0));
      __builtin_amdgcn_s_barrier();
      const char* tb = ring + (s & 1) * CC_TILE_B;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        V8 af[MF], bfr[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bfr[j] = *(const V8*)(tb + boff[kk] + j * 16 * CC_ROWB);
#pragma unroll
        for (int i = 0; i < MF; ++i)
          af[i] = *(const V8*)(wbuf + aoff[t & 1][kk] +
                               (i * 16 + t * CC_CB) * CC_ROWB);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = E8<elem_t>::mfma(af[i], bfr[j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
      __builtin_amdgcn_s_barrier();  // every wave done with slot s & 1
      if (s + 2 < nsteps) stage_tile(s & 1, c + (t + 2) / T, (t + 2) % T);
      if (t == T - 1 && c + 2 < nch) stage_win(c & 1, c + 2);
    }
  }

  // C tile through LDS: 16-byte row chunks with band, column and channel tails
  // (Nn % 8 == 0). Nothing is in flight: the last step waited for vmcnt(0).
  __syncthreads();
  elem_t* ct = (elem_t*)smem;
#pragma unroll
  for (int i = 0; i < MF; ++i)
    if (i < nf) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t col = wc + j * 16 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ct[(i * 16 + ((lane >> 4) << 2) + r) * CC_BN + col] =
              (elem_t)acc[i][j][r];
      }
    }
  __syncthreads();
  // round `it` covers tile row it * 16 + (tid >> 4): again one column per thread
  const uint32_t erow = tid >> 4, n = bn + (tid & 15) * 8;
  const uint32_t ej = j0 + (erow & 7);
  const uint32_t en = dW.div(ej);
  if (ej < NW && n < Nn) {
    elem_t* const ocol =
        out + (((size_t)en * H + h0) * W + dW.mod(ej, en)) * Nn + n;
    const size_t rowN = (size_t)W * Nn;
    for (uint32_t it = 0; it < nf; ++it) {
      const uint32_t hr = it * 2 + (erow >> 3);
      if (hr < hb)
        *(V8*)(ocol + hr * rowN) =
            *(const V8*)(ct + (it * 16 + erow) * CC_BN + (tid & 15) * 8);
    }
  }
}

// --------------------------------------------------------------- host side

// a zeroed 16-bit pattern reads as 0.0 in bf16 and fp16 alike
static const void* cc_zero_page(const at::Tensor& like) {
  static at::Tensor z;
  if (!z.defined() || z.device() != like.device())
    z = at::zeros({64}, like.options().dtype(at::kBFloat16));
  return z.data_ptr();
}

struct CcShape {
  long N, H, W, C, Ko, T;
};

// `a` is x (fwd) or dy (dgrad); both have the spatial size of the other
static CcShape cc_check(const char* op, const char* aname, const at::Tensor& a,
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
  CcShape s;
  s.N = a.size(0); s.H = a.size(2); s.W = a.size(3);
  s.Ko = w.size(0); s.C = w.size(1); s.T = w.size(2);
  TORCH_CHECK(w.size(3) == 1 && s.T > 1, op, ": the kernel must be Tx1, got ",
              s.T, "x", w.size(3));
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
  return s;
}

// out[n][h][w][Nn] from A [n][h][w][K] and B [Nn][T][K]
template <typename elem_t>
static void cc_launch(const char* op, const CcShape& s, const void* a,
                      const void* b, void* out, const void* zero, long K, long Nn) {
  // bands of near-equal height, the fewest the largest window class allows
  const long hb_max = CC_MAX_WRG * CC_GRP_H - (s.T - 1);
  const long bands = (s.H + hb_max - 1) / hb_max;
  const long hb_base = s.H / bands, hb_rem = s.H % bands;
  const long wimg = hb_base + (hb_rem ? 1 : 0) + s.T - 1;  // tallest window
  const long strips = (s.N * s.W + CC_CB - 1) / CC_CB;
  const long tiles_n = (Nn + CC_BN - 1) / CC_BN;
  const long grid = strips * bands * tiles_n;
  TORCH_CHECK(grid < (1ll << 31), op, ": grid of ", grid, " blocks too large");
  FastDiv dW;
  dW.init((uint32_t)s.W);
#define DTMX_CC_RUN(T_, G_)                                                     \
  colconv_kernel<elem_t, T_, G_>                                                \
      <<<(uint32_t)grid, CC_THREADS, 0, cc_stream()>>>(                         \
          (const elem_t*)a, (const elem_t*)b, (elem_t*)out, (const elem_t*)zero, \
          (uint32_t)(s.N * s.W), (uint32_t)s.H, (uint32_t)s.W, (uint32_t)K,     \
          (uint32_t)Nn, (uint32_t)(s.T * K), dW, (uint32_t)tiles_n,             \
          (uint32_t)bands, (uint32_t)hb_base, (uint32_t)hb_rem)
#define DTMX_CC_RUN_T(T_)                                   \
  do {                                                      \
    if (wimg <= 3 * CC_GRP_H) DTMX_CC_RUN(T_, 3);           \
    else if (wimg <= 4 * CC_GRP_H) DTMX_CC_RUN(T_, 4);      \
    else DTMX_CC_RUN(T_, 6);                                \
  } while (0)
  static_assert(CC_MAX_WRG == 6, "largest window buffer");
  if (s.T == 3) DTMX_CC_RUN_T(3);
  else if (s.T == 5) DTMX_CC_RUN_T(5);
  else DTMX_CC_RUN_T(7);
#undef DTMX_CC_RUN_T
#undef DTMX_CC_RUN
}

at::Tensor colconv_fwd(const at::Tensor& x, const at::Tensor& w) {
  const CcShape s = cc_check("colconv_fwd", "x", x, w, false);
  auto y = at::empty({s.N, s.Ko, s.H, s.W}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  const void* zero = cc_zero_page(x);
  DTMX_DISPATCH_16(x.scalar_type(), "colconv_fwd", {
    cc_launch<elem_t>("colconv_fwd", s, x.data_ptr(), w.data_ptr(), y.data_ptr(),
                      zero, s.C, s.Ko);
  });
  return y;
}

at::Tensor colconv_dgrad(const at::Tensor& dy, const at::Tensor& w) {
  const CcShape s = cc_check("colconv_dgrad", "dy", dy, w, true);
  auto dx = at::empty({s.N, s.C, s.H, s.W}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  auto wp = at::empty({s.C, s.T, s.Ko}, dy.options());
  const void* zero = cc_zero_page(dy);
  lineconv_pack(w, wp, s.C, s.Ko, s.T);
  DTMX_DISPATCH_16(dy.scalar_type(), "colconv_dgrad", {
    cc_launch<elem_t>("colconv_dgrad", s, dy.data_ptr(), wp.data_ptr(),
                      dx.data_ptr(), zero, s.Ko, s.C);
  });
  return dx;
}

}  // namespace dtmx
