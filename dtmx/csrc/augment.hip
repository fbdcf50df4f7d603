// Device-side image augmentation for gfx950: one pass from the decoded uint8
// records of a batch to the normalised 16-bit (or fp32) NHWC tensor the stem
// conv reads. (reference src/io/image_aug_default.cc resize / pad / crop /
// mirror / colour jitter / PCA lighting + iter_image_recordio_2.cc mean/std —
// the OpenCV chain of up to three resamplings and 8-bit intermediates is
// replaced by one bilinear gather and an fp32 colour chain.)
//
// src holds the batch's images back to back, HWC uint8 RGB, at any byte
// offset; geom[i] = {byte offset, H_i, W_i}. par[i] is the image's plan,
// AG_PAR floats:
//   0-5   affine map output -> source: u = a00(x+.5) + a01(y+.5) + a02,
//         v = a10(x+.5) + a11(y+.5) + a12; tap coordinates fx = u-.5, fy = v-.5
//   6-9   clamp box fx_lo, fx_hi, fy_lo, fy_hi applied to (fx, fy); +-inf = off
//   10    fill: what a bilinear tap outside [0,W-1] x [0,H-1] reads
//   11-13 alpha_b, alpha_c, alpha_s (1 = off)
//   14    order of (brightness, contrast, saturation): 0 bcs, 1 bsc, 2 cbs,
//         3 csb, 4 sbc, 5 scb
//   15-17 PCA add for R, G, B, in levels
//   18-19 spare
//
// Per pixel, all fp32 on [0,255], every stage ending in a clamp to [0,255]
// and no rounding to integers in between:
//   bilinear (x0 = floor(fx), weight fx-x0, four taps), the three colour
//   stages in the plan's order (v*ab; ac*v + (1-ac)*gmean; as*v +
//   (1-as)*gray(v), gray = .299R + .587G + .114B), + pca[c],
//   (v*(1/255) - mean[c]) / std[c], one convert at the store.
// gmean is the mean of gray over the image's TH*TW outputs as they stand when
// the contrast stage is reached. It needs a reduction, so when some
// alpha_c != 1 a pre-pass runs the same device function up to that stage and
// sums in a fixed order (thread-serial, wave shuffle tree, LDS, then the
// image's block partials in order): no float atomics, bit-identical run to
// run.
//
// A gather plus streaming-store bandwidth op. A work item is (image, chunk of
// AG_THREADS * AG_STRIP outputs); a block takes one item at a time, so plan
// and geometry loads are wave-uniform, and grid-strides over the items under
// a block cap. A thread owns AG_STRIP consecutive outputs of the image's
// flattened (y, x) order: 12 values, stored as three 8-byte (16-bit) or
// 16-byte (fp32) vectors when TH*TW % AG_STRIP == 0, element by element
// otherwise.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "dtmx_common.h"

namespace dtmx {

static hipStream_t ag_stream() { return at::hip::getCurrentHIPStream().stream(); }

constexpr int AG_THREADS = 256;
constexpr int AG_STRIP = 4;          // outputs per thread
constexpr int AG_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; grid-stride the rest
constexpr int AG_PAR = 20;           // floats per plan row
constexpr int AG_CHUNK = AG_THREADS * AG_STRIP;

// stage codes 0 brightness, 1 contrast, 2 saturation; order k's three stages
// sit in 2-bit fields of bits [6k, 6k+6)
constexpr uint64_t ag_order_bits(int s0, int s1, int s2, int k) {
  return (uint64_t)(s0 | (s1 << 2) | (s2 << 4)) << (6 * k);
}
constexpr uint64_t AG_ORDERS = ag_order_bits(0, 1, 2, 0) | ag_order_bits(0, 2, 1, 1) |
                               ag_order_bits(1, 0, 2, 2) | ag_order_bits(1, 2, 0, 3) |
                               ag_order_bits(2, 0, 1, 4) | ag_order_bits(2, 1, 0, 5);

struct AgNorm {
  float mean[3], std[3];
};

struct AgPlan {
  const uint8_t* img;
  int H, W;
  float a00, a01, a02, a10, a11, a12;
  float fx_lo, fx_hi, fy_lo, fy_hi;
  float fill, ab, ac, as;
  uint32_t stages;
  float pca[3];
};

__device__ __forceinline__ AgPlan ag_load_plan(const uint8_t* __restrict__ src,
                                               const int64_t* __restrict__ geom,
                                               const float* __restrict__ par,
                                               uint32_t n) {
  const int64_t* g = geom + (size_t)n * 3;
  const float* p = par + (size_t)n * AG_PAR;
  AgPlan P;
  P.img = src + g[0];
  P.H = (int)g[1];
  P.W = (int)g[2];
  P.a00 = p[0]; P.a01 = p[1]; P.a02 = p[2];
  P.a10 = p[3]; P.a11 = p[4]; P.a12 = p[5];
  P.fx_lo = p[6]; P.fx_hi = p[7]; P.fy_lo = p[8]; P.fy_hi = p[9];
  P.fill = p[10];
  P.ab = p[11]; P.ac = p[12]; P.as = p[13];
  int k = (int)p[14];
  k = k < 0 ? 0 : (k > 5 ? 5 : k);
  P.stages = (uint32_t)(AG_ORDERS >> (6 * k)) & 63u;
  P.pca[0] = p[15]; P.pca[1] = p[16]; P.pca[2] = p[17];
  return P;
}

__device__ __forceinline__ float ag_clamp(float v) {
  return fminf(fmaxf(v, 0.f), 255.f);
}

__device__ __forceinline__ float ag_gray(const float v[3]) {
  return 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
}

// tap (xi, yi), or fill outside the image
__device__ __forceinline__ void ag_tap(const AgPlan& P, int xi, int yi, float t[3]) {
  if ((uint32_t)xi < (uint32_t)P.W && (uint32_t)yi < (uint32_t)P.H) {
    const uint8_t* s = P.img + ((uint32_t)yi * (uint32_t)P.W + (uint32_t)xi) * 3u;
    t[0] = (float)s[0];
    t[1] = (float)s[1];
    t[2] = (float)s[2];
  } else {
    t[0] = t[1] = t[2] = P.fill;
  }
}

__device__ __forceinline__ void ag_sample(const AgPlan& P, uint32_t x, uint32_t y,
                                          float v[3]) {
  const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
  float fx = P.a00 * xc + P.a01 * yc + P.a02 - 0.5f;
  float fy = P.a10 * xc + P.a11 * yc + P.a12 - 0.5f;
  fx = fminf(fmaxf(fx, P.fx_lo), P.fx_hi);
  fy = fminf(fmaxf(fy, P.fy_lo), P.fy_hi);
  // every tap past one pixel outside reads fill anyway; this keeps the
  // float -> int conversion defined for any plan (far maps, inf, NaN)
  fx = fminf(fmaxf(fx, -2.f), (float)P.W + 1.f);
  fy = fminf(fmaxf(fy, -2.f), (float)P.H + 1.f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float wx = fx - x0f, wy = fy - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  float t00[3], t01[3], t10[3], t11[3];
  ag_tap(P, x0, y0, t00);
  ag_tap(P, x0 + 1, y0, t01);
  ag_tap(P, x0, y0 + 1, t10);
  ag_tap(P, x0 + 1, y0 + 1, t11);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = t00[c] + wx * (t01[c] - t00[c]);
    const float bot = t10[c] + wx * (t11[c] - t10[c]);
    v[c] = ag_clamp(top + wy * (bot - top));
  }
}

// Sample and run the colour stages. With TO_CONTRAST the chain stops where the
// contrast stage would run and returns gray there (the pre-pass' summand);
// otherwise v holds the pixel after all three stages.
template <bool TO_CONTRAST>
__device__ __forceinline__ float ag_pixel(const AgPlan& P, float gmean, uint32_t x,
                                          uint32_t y, float v[3]) {
  ag_sample(P, x, y, v);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t st = (P.stages >> (2 * i)) & 3u;
    if (st == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = ag_clamp(v[c] * P.ab);
    } else if (st == 1) {
      if (TO_CONTRAST) return ag_gray(v);
      const float add = (1.f - P.ac) * gmean;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = ag_clamp(P.ac * v[c] + add);
    } else {
      const float add = (1.f - P.as) * ag_gray(v);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = ag_clamp(P.as * v[c] + add);
    }
  }
  return 0.f;
}

// part[item] = sum of gray-at-the-contrast-stage over the item's outputs
__global__ __launch_bounds__(AG_THREADS) void augment_gray_partial_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ geom,
    const float* __restrict__ par, float* __restrict__ part, uint32_t THW,
    uint32_t TW, FastDiv dTW, FastDiv dChunks, uint32_t items) {
  __shared__ float wsum[AG_THREADS / DTMX_WAVE];
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t n = dChunks.div(it), chunk = dChunks.mod(it, n);
    const AgPlan P = ag_load_plan(src, geom, par, n);
    if (P.ac == 1.f) {  // block-uniform: contrast off, gmean unused
      if (threadIdx.x == 0) part[it] = 0.f;
      continue;
    }
    const uint32_t p0 = chunk * AG_CHUNK + threadIdx.x * AG_STRIP;
    float s = 0.f;
    if (p0 < THW) {
      uint32_t y = dTW.div(p0), x = dTW.mod(p0, y);
#pragma unroll
      for (int j = 0; j < AG_STRIP; ++j) {
        if (p0 + j < THW) {
          float v[3];
          s += ag_pixel<true>(P, 0.f, x, y, v);
        }
        if (++x == TW) { x = 0; ++y; }
      }
    }
#pragma unroll
    for (int d = DTMX_WAVE / 2; d >= 1; d >>= 1) s += __shfl_down(s, d, DTMX_WAVE);
    if ((threadIdx.x & (DTMX_WAVE - 1)) == 0) wsum[threadIdx.x / DTMX_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = wsum[0];
#pragma unroll
      for (int w = 1; w < AG_THREADS / DTMX_WAVE; ++w) t += wsum[w];
      part[it] = t;
    }
    __syncthreads();
  }
}

// gmean[n] = (the image's partials, summed in order) / THW
__global__ void augment_gray_final_kernel(const float* __restrict__ part,
                                          float* __restrict__ gmean, uint32_t B,
                                          uint32_t chunks, float thw) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const float* p = part + (size_t)n * chunks;
  float s = 0.f;
  for (uint32_t c = 0; c < chunks; ++c) s += p[c];
  gmean[n] = s / thw;
}

template <typename out_t>
__global__ __launch_bounds__(AG_THREADS) void augment_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ geom,
    const float* __restrict__ par, const float* __restrict__ gmean,
    out_t* __restrict__ out, AgNorm nm, uint32_t THW, uint32_t TW, FastDiv dTW,
    FastDiv dChunks, uint32_t items) {
  typedef out_t V4 __attribute__((ext_vector_type(4)));
  const bool vec = (THW % AG_STRIP) == 0;  // strips whole and vector-aligned
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t n = dChunks.div(it), chunk = dChunks.mod(it, n);
    const uint32_t p0 = chunk * AG_CHUNK + threadIdx.x * AG_STRIP;
    if (p0 >= THW) continue;
    const AgPlan P = ag_load_plan(src, geom, par, n);
    const float gm = gmean ? gmean[n] : 0.f;
    uint32_t y = dTW.div(p0), x = dTW.mod(p0, y);
    float o[AG_STRIP * 3];
#pragma unroll
    for (int j = 0; j < AG_STRIP; ++j) {
      float v[3] = {0.f, 0.f, 0.f};
      if (p0 + j < THW) ag_pixel<false>(P, gm, x, y, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // separate roundings, as the CPU path and the fp32 loader compute it:
        // exact-selection plans then agree with them bit for bit
#pragma clang fp contract(off)
        const float t = ag_clamp(v[c] + P.pca[c]);
        o[j * 3 + c] = (t * (1.f / 255.f) - nm.mean[c]) / nm.std[c];
      }
      if (++x == TW) { x = 0; ++y; }
    }
    out_t* dst = out + ((size_t)n * THW + p0) * 3;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        V4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (out_t)o[q * 4 + e];
        *(V4*)(dst + q * 4) = w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < AG_STRIP; ++j)
        if (p0 + j < THW) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[j * 3 + c] = (out_t)o[j * 3 + c];
        }
    }
  }
}

// --------------------------------------------------------------- host side

static void ag_check_host(const char* name, const at::Tensor& t, at::ScalarType st,
                          long B, long cols) {
  TORCH_CHECK(t.device().is_cpu() && t.scalar_type() == st && t.is_contiguous() &&
                  t.dim() == 2 && t.size(0) == B && t.size(1) == cols,
              "augment_batch: ", name, " must be a contiguous CPU ", st, " tensor of shape (",
              B, ", ", cols, ")");
}

// geom / par live on the device; geom_host / par_host are their host copies
// (CPU tensors of the same shape), read here for validation and to decide on
// the gmean pre-pass, never by a kernel. mean / std are 3-element CPU float
// tensors and travel as kernel arguments.
at::Tensor augment_batch(const at::Tensor& src, const at::Tensor& geom,
                         const at::Tensor& par, const at::Tensor& mean,
                         const at::Tensor& std_, long TH, long TW,
                         at::ScalarType out_dtype, const at::Tensor& geom_host,
                         const at::Tensor& par_host) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kByte && src.dim() == 1 &&
                  src.is_contiguous(),
              "augment_batch: src must be a contiguous 1-D uint8 GPU tensor");
  TORCH_CHECK(geom.is_cuda() && geom.scalar_type() == at::kLong && geom.dim() == 2 &&
                  geom.size(1) == 3 && geom.is_contiguous() &&
                  geom.get_device() == src.get_device(),
              "augment_batch: geom must be a contiguous (B, 3) int64 tensor on src's device");
  const long B = geom.size(0);
  TORCH_CHECK(B >= 1, "augment_batch: B must be >= 1");
  TORCH_CHECK(par.is_cuda() && par.scalar_type() == at::kFloat && par.dim() == 2 &&
                  par.size(0) == B && par.size(1) == AG_PAR && par.is_contiguous() &&
                  par.get_device() == src.get_device(),
              "augment_batch: par must be a contiguous (B, ", AG_PAR,
              ") float32 tensor on src's device");
  ag_check_host("geom_host", geom_host, at::kLong, B, 3);
  ag_check_host("par_host", par_host, at::kFloat, B, AG_PAR);
  TORCH_CHECK(TH >= 1 && TW >= 1, "augment_batch: TH and TW must be >= 1, got ", TH,
              " x ", TW);
  TORCH_CHECK(out_dtype == at::kBFloat16 || out_dtype == at::kHalf ||
                  out_dtype == at::kFloat,
              "augment_batch: out_dtype must be bfloat16, float16 or float32");
  TORCH_CHECK(B * 3 * TH * TW < (1ll << 31),
              "augment_batch: output too large (>= 2^31 elements)");
  AgNorm nm;
  for (int s = 0; s < 2; ++s) {
    const at::Tensor& t = s ? std_ : mean;
    TORCH_CHECK(t.device().is_cpu() && t.scalar_type() == at::kFloat && t.dim() == 1 &&
                    t.size(0) == 3 && t.is_contiguous(),
                "augment_batch: ", s ? "std" : "mean",
                " must be a contiguous 3-element CPU float32 tensor");
    for (int c = 0; c < 3; ++c) (s ? nm.std : nm.mean)[c] = t.data_ptr<float>()[c];
  }
  for (int c = 0; c < 3; ++c)
    TORCH_CHECK(nm.std[c] != 0.f, "augment_batch: std must be != 0, got std[", c, "] = 0");
  const int64_t* gh = geom_host.data_ptr<int64_t>();
  const float* ph = par_host.data_ptr<float>();
  bool contrast = false;
  for (long i = 0; i < B; ++i) {
    const int64_t off = gh[i * 3], H = gh[i * 3 + 1], W_ = gh[i * 3 + 2];
    TORCH_CHECK(H >= 1 && W_ >= 1, "augment_batch: image ", i, " must have H, W >= 1, got ",
                H, " x ", W_);
    // by division, so no product or sum can overflow
    const int64_t nb = src.numel();
    TORCH_CHECK(off >= 0 && off <= nb && H <= nb / W_ && H * W_ <= nb / 3 &&
                    off <= nb - H * W_ * 3,
                "augment_batch: image ", i, " (offset ", off, ", ", H, " x ", W_,
                " x 3) must lie inside src (", nb, " bytes)");
    // the kernel holds a 64-bit base per image and 32-bit offsets inside it
    TORCH_CHECK(H * W_ * 3 < (1ll << 31), "augment_batch: image ", i,
                " too large (H * W * 3 >= 2^31 bytes)");
    contrast |= ph[i * AG_PAR + 12] != 1.f;
  }

  auto out = at::empty({B, 3, TH, TW}, src.options().dtype(out_dtype),
                       at::MemoryFormat::ChannelsLast);
  const uint32_t THW = (uint32_t)(TH * TW);
  const uint32_t chunks = (THW + AG_CHUNK - 1) / AG_CHUNK;
  const uint32_t items = (uint32_t)B * chunks;  // <= out.numel() / 3
  const uint32_t grid = items < (uint32_t)AG_MAX_BLOCKS ? items : (uint32_t)AG_MAX_BLOCKS;
  FastDiv dTW, dChunks;
  dTW.init((uint32_t)TW);
  dChunks.init(chunks);
  auto sp = (const uint8_t*)src.data_ptr();
  auto gp = (const int64_t*)geom.data_ptr();
  auto pp = (const float*)par.data_ptr();
  const float* gm = nullptr;
  at::Tensor part, gmean;
  if (contrast) {
    part = at::empty({(long)items}, src.options().dtype(at::kFloat));
    gmean = at::empty({B}, src.options().dtype(at::kFloat));
    augment_gray_partial_kernel<<<grid, AG_THREADS, 0, ag_stream()>>>(
        sp, gp, pp, part.data_ptr<float>(), THW, (uint32_t)TW, dTW, dChunks, items);
    augment_gray_final_kernel<<<(B + 63) / 64, 64, 0, ag_stream()>>>(
        part.data_ptr<float>(), gmean.data_ptr<float>(), (uint32_t)B, chunks,
        (float)THW);
    gm = gmean.data_ptr<float>();
  }
  if (out_dtype == at::kBFloat16)
    augment_kernel<__bf16><<<grid, AG_THREADS, 0, ag_stream()>>>(
        sp, gp, pp, gm, (__bf16*)out.data_ptr(), nm, THW, (uint32_t)TW, dTW, dChunks, items);
  else if (out_dtype == at::kHalf)
    augment_kernel<_Float16><<<grid, AG_THREADS, 0, ag_stream()>>>(
        sp, gp, pp, gm, (_Float16*)out.data_ptr(), nm, THW, (uint32_t)TW, dTW, dChunks, items);
  else
    augment_kernel<float><<<grid, AG_THREADS, 0, ag_stream()>>>(
        sp, gp, pp, gm, (float*)out.data_ptr(), nm, THW, (uint32_t)TW, dTW, dChunks, items);
  return out;
}

}  // namespace dtmx
