// Line convolution weight gradient (1xT / Tx1) for gfx950, NHWC.
// (reference src/operator/nn/convolution.cu, kernel=(1,7) pad=(0,3) backward
// to the weight — the third pass of the lineconv.hip family.)
//
// x and dy share the flattened pixel index m = (n,h,w); with d = 1 (1xT) or
// d = W (Tx1) and pad = (T-1)/2:
//
//   dw[ko][t][c] = sum_m  dy[m][ko] . x[m + (t - pad) d][c] . valid(m, t)
//
// valid(m, t) = 0 when the tap coordinate of pixel m leaves [0, W) ([0, H) for
// Tx1): the forward kernel's border rule, which also keeps image n from
// reading n +- 1. dw is [Ko][T][C] in memory, the parameter's layout.
//
// A block (256 threads, 2 x 2 waves) owns BKO output channels x 64 input
// channels x all T taps and one slice of the pixels. All T accumulator sets
// are live at once, so the tile is sized by T: BKO = 128 at T = 3 (a wave
// owns 64 ko x 32 c, acc[3][4][2] f32x4 = 96 registers) and 64 at T = 5, 7
// (32 ko x 32 c, acc[T][2][2] = 80 / 112 registers). Per K-tile of 64 pixels
// the block stages, with global_load_lds,
//   dy   [64 px][BKO ko]            as one or two [64][64] parts, and
//   x    [64 + (T-1) d px][64 c]    the window, ONCE for all T taps,
// and every wave runs 2 x T x 2 FI v_mfma_f32_16x16x32 off them: the x fragment
// of tap t is the tap-0 read shifted by t d rows. conv_wgrad_hw gathers the
// same x pixels T times, with a FastDiv decode per 16-byte piece; here a
// window row is a pixel offset and staging has no division. Window rows before
// pixel 0 or past M, and channel tails, read the zero page.
//
// LDS rows are pixels (128 bytes = 64 channels): both operands are
// contraction-major and are read with ds_read_b64_tr_b16. One read of a wave
// covers rows {k .. k+3} and {k+8 .. k+11} per 32-lane half, 32 bytes (one
// chunk) each. Swizzle: chunk c of row r is stored at c ^ f(r),
// f(r) = bit1(r) | bit3(r) << 1, applied on the glds source side. Over
// {e, e+2, e+8, e+10} (the same-parity rows of a half, any e) bit 1 separates
// rows 2 apart and bit 3 rows 8 apart, so (r & 1, stored chunk) takes 8
// distinct values, the 64 banks, for EVERY k: the read stays conflict-free
// under any tap shift t d, not only multiples of 4 or 8 rows. f is taken from
// the shifted row per tap; + 32 rows (the second K half) leaves it unchanged.
//
// Border: the mask runs along the contraction. Per K-tile 64 threads decode
// one pixel each (one FastDiv decode) into its T validity bits and share them
// through a 128-byte LDS table; a lane reads the 16 pixels of its fragments
// back and, per tap, clears the invalid 16-bit elements of the x fragment in
// registers (a shift and a v_perm_b32 per pair). The centre tap needs none.
//
// Reduction over pixel slices is two-stage and deterministic: stage 1 writes
// fp32 part[slice][Ko][T][C], every element exactly once (no zero fill, no
// atomics); the finalize kernel adds the slices in index order, rounds once
// and writes dw. Bit-identical run to run.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <tuple>

#include "dtmx_common.h"

// The slice sums are plain fp32 arithmetic: keep the compiler from pairing
// them into packed fp32 instructions in this file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace dtmx {

static hipStream_t lw_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int LW_THREADS = 256;                // 4 waves, 2 (ko) x 2 (c)
constexpr int LW_BC = 64, LW_BK = 64;          // tile: input channels, pixels
constexpr int LW_ROWB = 128;                   // bytes of one LDS row (64 channels)
constexpr int LW_GRP = 32;                     // rows of one glds round of the block
constexpr int LW_GRP_B = LW_GRP * LW_ROWB;     // 4 KiB
constexpr int LW_PART_B = LW_BK * LW_ROWB;     // one [64 px][64 ko] dy part: 8 KiB
constexpr int LW_MAX_HALO = 256;               // (T-1) d, window rows
constexpr long LW_WS_BYTES = 32l << 20;        // fp32 workspace cap
constexpr int LW_FIN_THREADS = 256;

// 16-row ko fragments of a wave: all T taps' accumulators are live, 8 FI T
// registers per lane, so the ko tile shrinks as T grows (96 / 80 / 112)
constexpr int lw_fi(int T) { return T == 3 ? 4 : 2; }
constexpr int lw_bko(int T) { return 32 * lw_fi(T); }  // 2 waves along ko
// blocks per CU the registers and the LDS allow (WR: see the kernel)
constexpr int lw_blocks(int T, int WR) {
  return T == 3 ? (WR == 3 ? 2 : 1) : (WR <= 6 ? 2 : 1);
}

typedef __attribute__((ext_vector_type(2))) unsigned int lw_u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int lw_u32x4;

// chunk swizzle of LDS row r (see the file comment)
__device__ __forceinline__ uint32_t lw_f(uint32_t r) {
  return ((r >> 1) & 1) | (((r >> 3) & 1) << 1);
}

// s_waitcnt vmcnt(n), wave-uniform runtime n (the window's load count depends
// on W). Waiting for fewer loads in flight than asked is always safe.
__device__ __forceinline__ void lw_wait_vmcnt(uint32_t n) {
#define DTMX_LW_W(N_) \
  case N_: asm volatile("s_waitcnt vmcnt(" #N_ ")" ::: "memory"); break;
  switch (n) {
    DTMX_LW_W(1) DTMX_LW_W(2) DTMX_LW_W(3) DTMX_LW_W(4) DTMX_LW_W(5) DTMX_LW_W(6)
    DTMX_LW_W(7) DTMX_LW_W(8) DTMX_LW_W(9) DTMX_LW_W(10) DTMX_LW_W(11)
    DTMX_LW_W(12) DTMX_LW_W(13) DTMX_LW_W(14)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef DTMX_LW_W
}

// Four transposed reads, not waited for. In a 16-lane group lane 4a + b gives
// the address of row a, elements 4b .. 4b+3 of a [4 rows][16 elements] block;
// lane c receives column c of the four rows: four consecutive contraction
// indices of one output row / column, half an MFMA fragment.
__device__ __forceinline__ void lw_tr4(uint32_t a0, uint32_t a1, uint32_t a2,
                                       uint32_t a3, lw_u32x2 (&o)[4]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3])
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
}

// Waits until at most N LDS reads are in flight. The results ride through as
// in/out operands, so every use of a fragment depends on the wait that
// retires its read.
template <int N>
__device__ __forceinline__ void lw_wait_lgkm(lw_u32x2 (&o)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%4)"
               : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3])
               : "n"(N)
               : "memory");
}

// ------------------------------------------------------------ stage 1 kernel

// WR = 32-row glds rounds the window buffer holds: 3 (window <= 96 rows: 1xT
// and Tx1 halos up to 32), 6 (<= 192) or 10 (<= 320: the 256-row halo limit).
// LDS = 2 x (8 or 16 KiB dy + WR x 4 KiB window) + the two mask tables:
// 56.3 / 80.3 / 112.3 KiB at T = 3, 40.3 / 64.3 / 96.3 KiB at T = 5, 7.
// lw_blocks() is the blocks per CU that leaves room for.
//
// Load order, which the counted waits rely on (vmcnt retires in order): a
// stage is 2 or 4 dy loads then wgr window loads per thread, L in all;
//   prologue        stage 0, stage 1
//   top of tile i   s_waitcnt vmcnt(L) (stage i + 1 may be in flight; vmcnt(0)
//                   when there is none), s_barrier
//   end of tile i   s_barrier (every wave is done reading buffer i & 1), then
//                   stage i + 2 into buffer i & 1
// The mask table of a stage is written with it (ds_write, waited for before
// the writer's next barrier) and read after the top barrier of its tile.
template <typename elem_t, int T, int WR>
__global__ __launch_bounds__(LW_THREADS, lw_blocks(T, WR))
void lineconv_wgrad_partial_kernel(
    const elem_t* __restrict__ x, const elem_t* __restrict__ dy,
    float* __restrict__ part, const elem_t* __restrict__ zero, uint32_t M,
    uint32_t C, uint32_t Ko, uint32_t d, uint32_t L, uint32_t vertical,
    FastDiv dW, FastDiv dH, uint32_t tiles_c, uint32_t kt_base, uint32_t kt_rem) {
  using V8 = typename E8<elem_t>::v8;
  union Frag {
    V8 v;
    lw_u32x2 h[2];
  };
  constexpr int PAD = (T - 1) / 2;
  constexpr int FI = lw_fi(T), PARTS = FI / 2;  // dy parts of 64 ko
  constexpr uint32_t LW_BKO = lw_bko(T);
  constexpr uint32_t LW_DY_B = PARTS * LW_PART_B;
  constexpr uint32_t LW_DY_ROUNDS = LW_DY_B / LW_GRP_B;
  constexpr uint32_t STAGE_B = LW_DY_B + WR * LW_GRP_B;
  constexpr uint32_t TBL_OFF = 2 * STAGE_B;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_B + 2 * LW_BK * 2];

  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const uint32_t bko = (bid / tiles_c) * LW_BKO, bc = (bid % tiles_c) * LW_BC;
  // slice blockIdx.y owns K-tiles [kt0, kt0 + ktiles): kt_base each, one more
  // in the first kt_rem slices; slices <= K-tiles, so none is empty
  const uint32_t slice = blockIdx.y;
  const uint32_t kt0 = slice * kt_base + min(slice, kt_rem);
  const uint32_t ktiles = kt_base + (slice < kt_rem ? 1u : 0u);
  const uint32_t wrows = LW_BK + (T - 1) * d;            // window rows in use
  const uint32_t wgr = (wrows + LW_GRP - 1) / LW_GRP;    // glds rounds, <= WR
  const uint32_t nload = LW_DY_ROUNDS + wgr;

  // staging slot: round `it` covers LDS row it * 32 + srow, piece tid & 7;
  // 32 | the round stride, so one swizzle term serves every round
  const uint32_t srow = tid >> 3;
  const uint32_t sk = ((tid & 7) ^ (lw_f(srow) << 1)) << 3;  // source channel
  bool dy_ok[PARTS];
#pragma unroll
  for (int h = 0; h < PARTS; ++h) dy_ok[h] = bko + h * 64 + sk < Ko;
  const bool x_ok = bc + sk < C;

  auto stage = [&](uint32_t buf, uint32_t kt) {
    char* base = smem + buf * STAGE_B;
    const uint32_t mt = kt * LW_BK;
#pragma unroll
    for (int h = 0; h < PARTS; ++h)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const uint32_t m = mt + g * LW_GRP + srow;
        glds16(m < M && dy_ok[h] ? dy + (size_t)m * Ko + bko + h * 64 + sk : zero,
               base + h * LW_PART_B + g * LW_GRP_B + wave * 1024);
      }
    const int64_t m0 = (int64_t)mt - (int64_t)PAD * d + srow;  // pixel of row srow
    for (uint32_t it = 0; it < wgr; ++it) {
      const int64_t m = m0 + it * LW_GRP;
      const bool ok = m >= 0 && m < (int64_t)M && x_ok && it * LW_GRP + srow < wrows;
      glds16(ok ? x + (size_t)m * C + bc + sk : zero,
             base + LW_DY_B + it * LW_GRP_B + wave * 1024);
    }
    // tap validity of pixel mt + tid: bit t set when tap t stays in the image
    if (tid < LW_BK) {
      const uint32_t m = mt + tid;
      uint32_t bits = 0;
      if (m < M) {
        const uint32_t q = dW.div(m);
        const uint32_t pos = vertical ? dH.mod(q, dH.div(q)) : dW.mod(m, q);
#pragma unroll
        for (int t = 0; t < T; ++t)
          bits |= (uint32_t)(pos + t - PAD < L) << t;  // unsigned: < 0 wraps high
      }
      *(unsigned short*)(smem + TBL_OFF + buf * (LW_BK * 2) + tid * 2) =
          (unsigned short)bits;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  };

  // fragment read addresses (bytes from a stage's base, K half 0). Lane
  // 16 grp + 4 q + p supplies row 8 grp + q (lo) or + 4 (hi), bytes 8 p of a
  // chunk; dy rows are never shifted, x rows move by t d per tap.
  const uint32_t wr = wave >> 1, wc = wave & 1;  // ko, c half of the block tile
  const uint32_t grp = lane >> 4, q = (lane >> 2) & 3, p8 = (lane & 3) * 8;
  const uint32_t row0 = grp * 8 + q;
  uint32_t a_rd[FI];
#pragma unroll
  for (uint32_t i = 0; i < FI; ++i) {  // lo; hi = + 4 rows: bits 1, 3 unchanged
    const uint32_t kl = wr * 16 * FI + i * 16;  // ko inside the block tile
    a_rd[i] = (kl >> 6) * LW_PART_B + row0 * LW_ROWB +
              ((((kl >> 4) & 3) ^ lw_f(row0)) << 5) + p8;
  }
  uint32_t x_rd[T][2][2];  // [tap][lo, hi][c fragment]
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (uint32_t hi = 0; hi < 2; ++hi) {
      const uint32_t r = row0 + hi * 4 + t * d;
#pragma unroll
      for (uint32_t j = 0; j < 2; ++j)
        x_rd[t][hi][j] =
            LW_DY_B + r * LW_ROWB + (((wc * 2 + j) ^ lw_f(r)) << 5) + p8;
    }
  const uint32_t smem0 = (uint32_t)(uintptr_t)smem;

  f32x4 acc[T][FI][2];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, kt0);
  if (ktiles > 1) stage(1, kt0 + 1);

  for (uint32_t it = 0; it < ktiles; ++it) {
    lw_wait_vmcnt(it + 1 < ktiles ? nload : 0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const uint32_t buf = it & 1;
    const uint32_t sb = smem0 + buf * STAGE_B;
    // validity of this lane's fragment pixels 32 kk + 8 grp + (0 .. 7): one
    // 16-bit entry per pixel, two pixels per register
    lw_u32x4 pm[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      pm[kk] = *(const lw_u32x4*)(smem + TBL_OFF + buf * (LW_BK * 2) +
                                  (kk * 32 + grp * 8) * 2);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const uint32_t kb = sb + kk * 32 * LW_ROWB;
      // dy: fragment i lo at [i], hi at [FI + i]; xb[slot]: lo j0, lo j1,
      // hi j0, hi j1
      lw_u32x2 ad[FI / 2][4], xb[2][4];
      if constexpr (FI == 4) {
        lw_tr4(kb + a_rd[0], kb + a_rd[1], kb + a_rd[2], kb + a_rd[3], ad[0]);
        lw_tr4(kb + a_rd[0] + 4 * LW_ROWB, kb + a_rd[1] + 4 * LW_ROWB,
               kb + a_rd[2] + 4 * LW_ROWB, kb + a_rd[3] + 4 * LW_ROWB, ad[1]);
      } else {
        lw_tr4(kb + a_rd[0], kb + a_rd[1], kb + a_rd[0] + 4 * LW_ROWB,
               kb + a_rd[1] + 4 * LW_ROWB, ad[0]);
      }
      lw_tr4(kb + x_rd[0][0][0], kb + x_rd[0][0][1], kb + x_rd[0][1][0],
             kb + x_rd[0][1][1], xb[0]);
      Frag af[FI];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        lw_u32x2(&cur)[4] = xb[t & 1];
        if (t == 0) {  // dy done, tap 0 may be in flight: at most 12 reads out
#pragma unroll
          for (int u = 0; u < FI / 2; ++u) lw_wait_lgkm<4>(ad[u]);
        }
        if (t + 1 < T) {  // tap t + 1 flies under tap t's mask and MFMAs
          lw_tr4(kb + x_rd[t + 1][0][0], kb + x_rd[t + 1][0][1],
                 kb + x_rd[t + 1][1][0], kb + x_rd[t + 1][1][1], xb[(t + 1) & 1]);
          lw_wait_lgkm<4>(cur);
        } else {
          lw_wait_lgkm<0>(cur);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the MFMAs below the wait
        if (t == 0) {
#pragma unroll
          for (int i = 0; i < FI; ++i) {
            af[i].h[0] = ad[i / 4][i % 4];
            af[i].h[1] = ad[(FI + i) / 4][(FI + i) % 4];
          }
        }
        if (t != PAD) {
          // element pair e of half hi is pixels 4 hi + 2 e, + 1: bit t of each
          // 16-bit entry moves to its sign and v_perm_b32 spreads the two
          // signs over their halves of the register
#pragma unroll
          for (int hi = 0; hi < 2; ++hi)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const uint32_t s = pm[kk][hi * 2 + e] << (15 - t);
              const uint32_t mk = __builtin_amdgcn_perm(s, s, 0x09090808u);
              cur[hi * 2][e] &= mk;
              cur[hi * 2 + 1][e] &= mk;
            }
        }
        Frag bf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bf[j].h[0] = cur[j];
          bf[j].h[1] = cur[2 + j];
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[t][i][j] = E8<elem_t>::mfma(af[i].v, bf[j].v, acc[t][i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __builtin_amdgcn_s_barrier();  // every wave done with buffer it & 1
    if (it + 2 < ktiles) stage(buf, kt0 + it + 2);
  }

  // D row 4 grp + r of fragment i is channel bko + 16 FI wr + 16 i + 4 grp + r,
  // column lane & 15 of fragment j is input channel bc + 32 wc + 16 j + ...
  float* const pbase = part + (size_t)slice * Ko * T * C;
  const uint32_t c0 = bc + wc * 32 + (lane & 15);
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t ko = bko + wr * 16 * FI + i * 16 + grp * 4 + r;
      if (ko >= Ko) continue;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (c0 + j * 16 < C)
            pbase[((size_t)ko * T + t) * C + c0 + j * 16] = acc[t][i][j][r];
    }
}

// ------------------------------------------------------------ stage 2 kernel

// Thread i owns the 8 consecutive outputs 8 i .. 8 i + 7 of dw [Ko][T][C]
// (C % 8 == 0: one 16-byte store): adds part[0 .. NS) in index order.
template <typename elem_t>
__global__ __launch_bounds__(LW_FIN_THREADS) void lineconv_wgrad_finalize_kernel(
    const float* __restrict__ part, elem_t* __restrict__ dw, uint32_t n8,
    uint32_t NS) {
  using V8 = typename E8<elem_t>::v8;
  const uint32_t i = blockIdx.x * LW_FIN_THREADS + threadIdx.x;
  if (i >= n8) return;
  const size_t n = (size_t)n8 * 8;
  const float* p = part + (size_t)i * 8;
  f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  for (uint32_t s = 1; s < NS; ++s) {
    p += n;
    const f32x4 u = *(const f32x4*)p, v = *(const f32x4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] += u[e];
      b[e] += v[e];
    }
  }
  V8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = (elem_t)a[e];
    o[4 + e] = (elem_t)b[e];
  }
  *(V8*)(dw + (size_t)i * 8) = o;
}

// --------------------------------------------------------------- host side

// a zeroed 16-bit pattern reads as 0.0 in bf16 and fp16 alike
static const void* lw_zero_page(const at::Tensor& like) {
  static at::Tensor z;
  if (!z.defined() || z.device() != like.device())
    z = at::zeros({64}, like.options().dtype(at::kBFloat16));
  return z.data_ptr();
}

static long lw_ktiles(long N, long H, long W) {
  return (N * H * W + LW_BK - 1) / LW_BK;
}

// (tile class, slices): the class is the window buffer's 32-row rounds (3, 6
// or 10). Slices fill the CUs (two blocks each where the class allows it)
// while the fp32 workspace stays under its cap and every slice has a K-tile.
std::tuple<long, long> lineconv_wgrad_plan(long Ko, long C, long T, bool vertical,
                                           long N, long H, long W) {
  TORCH_CHECK(Ko > 0 && C > 0 && N > 0 && H > 0 && W > 0 &&
                  (T == 3 || T == 5 || T == 7),
              "lineconv_wgrad_plan: positive sizes and T in {3, 5, 7} required");
  const long wrows = LW_BK + (T - 1) * (vertical ? W : 1);
  const long cls = wrows <= 3 * LW_GRP ? 3 : wrows <= 6 * LW_GRP ? 6 : 10;
  const long bko = lw_bko((int)T);
  const long tiles = ((Ko + bko - 1) / bko) * ((C + LW_BC - 1) / LW_BC);
  const long blocks = lw_blocks((int)T, (int)cls) * DTMX_CUS;
  const long fit = std::max<long>(1, LW_WS_BYTES / (Ko * T * C * 4));
  const long slices = std::max<long>(
      1, std::min({(blocks + tiles - 1) / tiles, fit, lw_ktiles(N, H, W)}));
  return {cls, slices};
}

at::Tensor lineconv_wgrad(const at::Tensor& x, const at::Tensor& dy, long T,
                          bool vertical, long slices) {
  const char* op = "lineconv_wgrad";
  TORCH_CHECK(x.is_cuda() && (x.scalar_type() == at::kBFloat16 ||
                              x.scalar_type() == at::kHalf),
              op, ": x must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == x.scalar_type() &&
                  dy.device() == x.device(),
              op, ": dy must be on the device of x and of its dtype");
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4 && x.numel() > 0 && dy.numel() > 0 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": x and dy must be non-empty 4-D NHWC (channels_last) tensors");
  TORCH_CHECK(T == 3 || T == 5 || T == 7, op, ": T must be 3, 5 or 7, got ", T);
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long Ko = dy.size(1);
  // stride 1 and same padding on the tap axis: dy has the spatial size of x
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == H && dy.size(3) == W, op,
              ": dy must have the batch and spatial size of x (stride 1, padding "
              "(T-1)/2 on the tap axis), want ", N, "x", Ko, "x", H, "x", W);
  TORCH_CHECK(C % 8 == 0, op, ": C % 8 == 0 required, got C = ", C);
  TORCH_CHECK(Ko % 8 == 0, op, ": Ko % 8 == 0 required, got Ko = ", Ko);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)dy.data_ptr() % 16 == 0,
              op, ": x and dy must be 16-byte aligned");
  TORCH_CHECK(N * H * W < (1ll << 31), op, ": N*H*W < 2^31 required, got ",
              N * H * W);
  TORCH_CHECK(Ko * T * C < (1ll << 31), op, ": dw too large (>= 2^31 elements)");
  TORCH_CHECK(!vertical || (T - 1) * W <= LW_MAX_HALO, op,
              ": Tx1 needs a halo (T-1)*W of at most ", LW_MAX_HALO, " rows, got ",
              (T - 1) * W);
  const long ktiles = lw_ktiles(N, H, W);
  const auto plan = lineconv_wgrad_plan(Ko, C, T, vertical, N, H, W);
  const long cls = std::get<0>(plan);
  TORCH_CHECK(slices >= 0 && slices <= ktiles, op, ": 0 <= slices <= ceil(N*H*W / ",
              LW_BK, ") = ", ktiles, " required, got ", slices);
  const long NS = slices > 0 ? slices : std::get<1>(plan);
  TORCH_CHECK(NS * Ko * T * C * 4 <= std::max<long>(LW_WS_BYTES, Ko * T * C * 4), op,
              ": slices * Ko*T*C*4 bytes must stay under the ", LW_WS_BYTES >> 20,
              " MiB workspace cap, got slices = ", NS);

  auto part = at::empty({NS, Ko, T, C}, x.options().dtype(at::kFloat));
  auto dwm = vertical ? at::empty({Ko, T, 1, C}, x.options())
                      : at::empty({Ko, 1, T, C}, x.options());
  const void* zero = lw_zero_page(x);
  const uint32_t M = (uint32_t)(N * H * W);
  const uint32_t d = vertical ? (uint32_t)W : 1u;
  const uint32_t L = (uint32_t)(vertical ? H : W);
  FastDiv dW, dH;
  dW.init((uint32_t)W);
  dH.init((uint32_t)H);
  const uint32_t tiles_c = (uint32_t)((C + LW_BC - 1) / LW_BC);
  const uint32_t tiles = (uint32_t)((Ko + lw_bko((int)T) - 1) / lw_bko((int)T)) * tiles_c;
  dim3 grid(tiles, (uint32_t)NS);
  const uint32_t n8 = (uint32_t)(Ko * T * C / 8);
#define DTMX_LW_RUN(T_, G_)                                                       \
  lineconv_wgrad_partial_kernel<elem_t, T_, G_>                                   \
      <<<grid, LW_THREADS, 0, lw_stream()>>>(                                     \
          (const elem_t*)x.data_ptr(), (const elem_t*)dy.data_ptr(),              \
          part.data_ptr<float>(), (const elem_t*)zero, M, (uint32_t)C,            \
          (uint32_t)Ko, d, L, vertical ? 1u : 0u, dW, dH, tiles_c,                \
          (uint32_t)(ktiles / NS), (uint32_t)(ktiles % NS))
#define DTMX_LW_RUN_T(T_)                    \
  do {                                       \
    if (cls == 3) DTMX_LW_RUN(T_, 3);        \
    else if (cls == 6) DTMX_LW_RUN(T_, 6);   \
    else DTMX_LW_RUN(T_, 10);                \
  } while (0)
  static_assert(LW_BK + LW_MAX_HALO <= 10 * LW_GRP, "largest window buffer");
  DTMX_DISPATCH_16(x.scalar_type(), op, {
    if (T == 3) DTMX_LW_RUN_T(3);
    else if (T == 5) DTMX_LW_RUN_T(5);
    else DTMX_LW_RUN_T(7);
    lineconv_wgrad_finalize_kernel<elem_t>
        <<<(n8 + LW_FIN_THREADS - 1) / LW_FIN_THREADS, LW_FIN_THREADS, 0,
           lw_stream()>>>(part.data_ptr<float>(), (elem_t*)dwm.data_ptr(), n8,
                          (uint32_t)NS);
  });
#undef DTMX_LW_RUN_T
#undef DTMX_LW_RUN
  return dwm.permute({0, 3, 1, 2});  // logical (Ko,C,R,S), channels_last
}

}  // namespace dtmx

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
