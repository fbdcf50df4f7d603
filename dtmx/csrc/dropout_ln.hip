// Dropout (counter-based RNG mask + scale) and LayerNorm fwd/bwd for gfx950.
// Reference behavior: src/operator/nn/dropout.cu (mask-gen + scale, p = drop
// probability, train-only) and src/operator/nn/layer_norm.cu (row mean/var
// normalize with gamma/beta). MI355X-native design: stateless splitmix64
// counter RNG (no cuRAND state arrays), uint8 mask, fp32 accumulation;
// LayerNorm is one 256-thread block per row with wave shuffle reductions.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"

namespace dtmx {

static hipStream_t dl_stream() { return at::hip::getCurrentHIPStream().stream(); }

// splitmix64: high-quality stateless hash of (seed, counter)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// ---- dropout --------------------------------------------------------------
// One hash yields 64 random bits -> two 32-bit uniforms; process 2 elems/iter.
template <typename elem_t>
__global__ void dropout_fwd_kernel(const elem_t* __restrict__ x,
                                   elem_t* __restrict__ y,
                                   uint8_t* __restrict__ mask, size_t n,
                                   float p, float inv_keep, uint64_t seed) {
  size_t i2 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint32_t thresh = (uint32_t)(p * 4294967296.0);  // drop if r < thresh
  for (; i2 * 2 < n; i2 += stride) {
    uint64_t r = splitmix64(seed ^ (i2 * 0x5851f42d4c957f2dull));
    size_t i = i2 * 2;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if (i + e >= n) break;
      uint32_t u = (uint32_t)(r >> (32 * e));
      uint8_t keep = u >= thresh;
      mask[i + e] = keep;
      y[i + e] = keep ? (elem_t)((float)x[i + e] * inv_keep) : (elem_t)0.f;
    }
  }
}

template <typename elem_t>
__global__ void dropout_bwd_kernel(const elem_t* __restrict__ dy,
                                   const uint8_t* __restrict__ mask,
                                   elem_t* __restrict__ dx, size_t n,
                                   float inv_keep) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    dx[i] = mask[i] ? (elem_t)((float)dy[i] * inv_keep) : (elem_t)0.f;
}

std::vector<at::Tensor> dropout_fwd(const at::Tensor& x, double p, int64_t seed) {
  TORCH_CHECK(x.is_cuda(), "dropout_fwd: CUDA tensor required");
  auto xc = x.contiguous();
  size_t n = xc.numel();
  auto y = at::empty_like(xc);
  auto mask = at::empty({(long)n}, xc.options().dtype(at::kByte));
  float inv_keep = 1.f / (1.f - (float)p);
  uint32_t blocks = std::min<size_t>((n / 2 + 255) / 256 + 1, 4096);
  DTMX_DISPATCH_16(xc.scalar_type(), "dropout_fwd", {
    dropout_fwd_kernel<<<blocks, 256, 0, dl_stream()>>>(
        (const elem_t*)xc.data_ptr(), (elem_t*)y.data_ptr(),
        mask.data_ptr<uint8_t>(), n, (float)p, inv_keep, (uint64_t)seed);
  });
  return {y, mask};
}

at::Tensor dropout_bwd(const at::Tensor& dy, const at::Tensor& mask, double p) {
  auto dyc = dy.contiguous();
  size_t n = dyc.numel();
  auto dx = at::empty_like(dyc);
  float inv_keep = 1.f / (1.f - (float)p);
  uint32_t blocks = std::min<size_t>((n + 255) / 256, 4096);
  DTMX_DISPATCH_16(dyc.scalar_type(), "dropout_bwd", {
    dropout_bwd_kernel<<<blocks, 256, 0, dl_stream()>>>(
        (const elem_t*)dyc.data_ptr(), mask.data_ptr<uint8_t>(),
        (elem_t*)dx.data_ptr(), n, inv_keep);
  });
  return dx;
}

// ---- layernorm ------------------------------------------------------------
// One 256-thread block per row. The row statistics are taken in two passes
// in fp64: the mean first, then the centred sum of squares. The one-pass
// fp32 form var = sum(x^2)/D - mean^2 cancels on rows whose mean is large
// against their spread (rstd off by 0.9 % on fp16 rows 64 + k/16), and an
// fp32 mean alone leaves (x - mean) wrong where x is close to the mean. The
// row is cache-resident and LN is off the hot path, so the second pass and
// the fp64 arithmetic are free; mean and rstd are saved as fp64 for backward.

// sum of v over the block's 256 threads (4 waves), result in every thread
__device__ __forceinline__ double ln_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();  // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <typename elem_t>
__global__ void ln_fwd_kernel(const elem_t* __restrict__ x,
                              const float* __restrict__ gamma,
                              const float* __restrict__ beta,
                              elem_t* __restrict__ y, double* __restrict__ mean,
                              double* __restrict__ rstd, uint32_t D, double eps) {
  const uint32_t row = blockIdx.x, t = threadIdx.x;
  const elem_t* in = x + (size_t)row * D;
  elem_t* out = y + (size_t)row * D;
  __shared__ double red[4];

  double s = 0.0;
  for (uint32_t i = t; i < D; i += 256) s += (double)(float)in[i];
  const double m = ln_block_sum(s, red) / D;
  double css = 0.0;
  for (uint32_t i = t; i < D; i += 256) {
    double d = (double)(float)in[i] - m;
    css += d * d;
  }
  const double var = ln_block_sum(css, red) / D;
  const double rs = 1.0 / sqrt(var + eps);
  if (t == 0) {
    mean[row] = m;
    rstd[row] = rs;
  }
  for (uint32_t i = t; i < D; i += 256) {
    float xh = (float)(((double)(float)in[i] - m) * rs);
    out[i] = (elem_t)(xh * gamma[i] + beta[i]);
  }
}

// dx = rstd * (g - mean_row(g) - xhat * mean_row(g * xhat)),  g = dy * gamma
// dgamma/dbeta accumulated across rows with fp32 atomics (LN is not on the
// ResNet hot path; atomics keep it one pass). Each dgamma term dy * xhat is
// formed in fp64 and rounded once, so the only fp32 errors are that rounding
// and the adds: within B * 2^-23 * sum|terms|.
template <typename elem_t>
__global__ void ln_bwd_kernel(const elem_t* __restrict__ x,
                              const elem_t* __restrict__ dy,
                              const float* __restrict__ gamma,
                              const double* __restrict__ mean,
                              const double* __restrict__ rstd,
                              elem_t* __restrict__ dx,
                              float* __restrict__ dgamma,
                              float* __restrict__ dbeta, uint32_t D) {
  const uint32_t row = blockIdx.x, t = threadIdx.x;
  const elem_t* xr = x + (size_t)row * D;
  const elem_t* dyr = dy + (size_t)row * D;
  elem_t* dxr = dx + (size_t)row * D;
  const double m = mean[row], rs = rstd[row];
  __shared__ double red[4];

  double s1 = 0.0, s2 = 0.0;
  for (uint32_t i = t; i < D; i += 256) {
    double xh = ((double)(float)xr[i] - m) * rs;
    double g = (double)(float)dyr[i] * (double)gamma[i];
    s1 += g;
    s2 += g * xh;
    atomicAdd(&dgamma[i], (float)((double)(float)dyr[i] * xh));
    atomicAdd(&dbeta[i], (float)dyr[i]);
  }
  s1 = ln_block_sum(s1, red) / D;
  s2 = ln_block_sum(s2, red) / D;
  for (uint32_t i = t; i < D; i += 256) {
    double xh = ((double)(float)xr[i] - m) * rs;
    double g = (double)(float)dyr[i] * (double)gamma[i];
    dxr[i] = (elem_t)(float)(rs * (g - s1 - xh * s2));
  }
}

std::vector<at::Tensor> layer_norm_fwd(const at::Tensor& x, const at::Tensor& gamma,
                                       const at::Tensor& beta, double eps) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "layer_norm_fwd: 2D CUDA tensor");
  auto xc = x.contiguous();
  uint32_t B = xc.size(0), D = xc.size(1);
  auto gf = gamma.to(at::kFloat).contiguous();
  auto bf = beta.to(at::kFloat).contiguous();
  auto y = at::empty_like(xc);
  auto mean = at::empty({(long)B}, xc.options().dtype(at::kDouble));
  auto rstd = at::empty({(long)B}, xc.options().dtype(at::kDouble));
  DTMX_DISPATCH_16(xc.scalar_type(), "layer_norm_fwd", {
    ln_fwd_kernel<<<B, 256, 0, dl_stream()>>>(
        (const elem_t*)xc.data_ptr(), gf.data_ptr<float>(), bf.data_ptr<float>(),
        (elem_t*)y.data_ptr(), mean.data_ptr<double>(), rstd.data_ptr<double>(),
        D, eps);
  });
  return {y, mean, rstd};
}

std::vector<at::Tensor> layer_norm_bwd(const at::Tensor& x, const at::Tensor& dy,
                                       const at::Tensor& gamma,
                                       const at::Tensor& mean,
                                       const at::Tensor& rstd) {
  auto xc = x.contiguous();
  auto dyc = dy.contiguous();
  uint32_t B = xc.size(0), D = xc.size(1);
  TORCH_CHECK(mean.scalar_type() == at::kDouble && rstd.scalar_type() == at::kDouble &&
                  mean.is_contiguous() && rstd.is_contiguous() &&
                  mean.numel() == B && rstd.numel() == B,
              "layer_norm_bwd: mean/rstd must be the fp64 [B] tensors of layer_norm_fwd");
  TORCH_CHECK(dyc.sizes() == xc.sizes() && dyc.scalar_type() == xc.scalar_type(),
              "layer_norm_bwd: dy must match x");
  auto gf = gamma.to(at::kFloat).contiguous();
  auto dx = at::empty_like(xc);
  auto dgamma = at::zeros({(long)D}, xc.options().dtype(at::kFloat));
  auto dbeta = at::zeros({(long)D}, xc.options().dtype(at::kFloat));
  DTMX_DISPATCH_16(xc.scalar_type(), "layer_norm_bwd", {
    ln_bwd_kernel<<<B, 256, 0, dl_stream()>>>(
        (const elem_t*)xc.data_ptr(), (const elem_t*)dyc.data_ptr(),
        gf.data_ptr<float>(), mean.data_ptr<double>(), rstd.data_ptr<double>(),
        (elem_t*)dx.data_ptr(), dgamma.data_ptr<float>(),
        dbeta.data_ptr<float>(), D);
  });
  return {dx, dgamma, dbeta};
}

}  // namespace dtmx
