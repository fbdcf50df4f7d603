// Backward of the fused bias + ReLU epilogue (VGG / AlexNet / GoogLeNet convs
// and hidden FCs): one pass over (dy, y) writes the masked gradient
//   g[r][c] = (float)y[r][c] > 0 ? dy[r][c] : 0        (relu_bwd's predicate)
// and the bias gradient db32[c] = sum_r g[r][c] in fp32. Without ReLU the
// pass is a column sum of dy alone: y is not read and no g is written.
//
// The operands are one dense buffer viewed as [rows][C] (an NHWC activation
// with rows = N*P*Q, or an (M, N) FC output), C % 8 == 0.
//
// Fixed-column geometry, as the BN statistics kernels: a thread owns ONE
// 16-byte channel vector for its whole walk and keeps 8 fp32 sums in
// registers. A block is BC columns x L row lanes (BC * L <= 256):
//   C/8 <= 256:  BC = C/8, L = 256 / BC, grid.y = 1   (thread t: column
//                t % BC, lane t / BC — a wave reads whole consecutive rows)
//   C/8 >  256:  BC = 64,  L = 4, grid.y = ceil(C/8 / 64)  (FC, C = 4096)
// grid.x row walkers (at most BA_WALKERS) deal the row groups of L rows
// round-robin; a thread issues BA_UNROLL of its groups at once. At the end
// the block folds its L lanes through 8 KB of LDS, lane 0 first — a linear
// fold over lanes of the SAME column, so a C/8 that is no power of two
// (3, 5, 26, 66 vectors) mixes nothing — and writes its exclusive fp32 row
// segment of a [grid.x][C] slab. bias_act_bwd_reduce_kernel adds the slab
// rows of each channel, block 0 first. No atomics anywhere: db32 is
// bit-identical run to run, and every slab element is written, so the
// workspace is at::empty.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "dtmx_common.h"

namespace dtmx {

constexpr int BA_THREADS = 256;
constexpr int BA_WALKERS = 256;  // one block per CU and per column group
constexpr int BA_UNROLL = 4;

// The sums are plain fp32 adds that the compiler would pair into packed fp32
// instructions; as in stemconv.hip and dwconv_fwd_stats_kernel, the
// statistics kernels are built without them. The attribute is per function.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// __syncthreads() with builtins only: the headers' device functions carry the
// default target features and are not inlined into this region.
__device__ __forceinline__ void ba_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <typename elem_t, bool RELU>
__global__ __launch_bounds__(BA_THREADS) void bias_act_bwd_kernel(
    const elem_t* __restrict__ dy, const elem_t* __restrict__ y,
    elem_t* __restrict__ g, float* __restrict__ slab, uint32_t rows,
    uint32_t cvecs, uint32_t bc, uint32_t lanes) {
  using V8 = typename E8<elem_t>::v8;
  __shared__ float red[BA_THREADS * 8];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid / bc, col = tid - lane * bc;
  const uint32_t cv0 = blockIdx.y * bc;  // first channel vector of the block
  const uint32_t C = cvecs * 8;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  if (lane < lanes && cv0 + col < cvecs) {
    const size_t coff = (size_t)(cv0 + col) * 8;
    // rows < 2^28 and step <= 2^16, so r + BA_UNROLL * step stays in 32 bits
    const uint32_t step = gridDim.x * lanes;
    for (uint32_t r0 = blockIdx.x * lanes + lane; r0 < rows;
         r0 += BA_UNROLL * step) {
      V8 d[BA_UNROLL], v[BA_UNROLL];
#pragma unroll
      for (int u = 0; u < BA_UNROLL; ++u) {
        const uint32_t r = r0 + u * step;
        const V8 z = {};
        d[u] = z;
        v[u] = z;
        if (r < rows) {
          d[u] = *(const V8*)(dy + (size_t)r * C + coff);
          if (RELU) v[u] = *(const V8*)(y + (size_t)r * C + coff);
        }
      }
#pragma unroll
      for (int u = 0; u < BA_UNROLL; ++u) {
        const uint32_t r = r0 + u * step;
        if (RELU) {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            d[u][e] = (float)v[u][e] > 0.f ? d[u][e] : (elem_t)0.f;
          if (r < rows) *(V8*)(g + (size_t)r * C + coff) = d[u];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (float)d[u][e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tid * 8 + e] = s[e];
  ba_barrier();
  // f = (column, element) of the block; lane l of it sits at red[l*bc*8 + f]
  const uint32_t width = bc * 8;
  for (uint32_t f = tid; f < width; f += BA_THREADS) {
    if (cv0 * 8 + f >= C) break;
    float t = 0.f;
    for (uint32_t l = 0; l < lanes; ++l) t += red[l * width + f];
    slab[(size_t)blockIdx.x * C + cv0 * 8 + f] = t;
  }
}

// db[c] = sum of slab[.][c] in a fixed order: a block takes BA_RCOLS channels
// x BA_RLANES lanes, lane l adds slab rows l, l + BA_RLANES, ... in that order
// (four loads in flight; a wave reads two 128-byte row segments at a time),
// then the lanes fold through LDS, lane 0 first. A single thread a channel
// would walk up to 256 rows in one dependent chain.
constexpr int BA_RCOLS = 32;
constexpr int BA_RLANES = BA_THREADS / BA_RCOLS;

__global__ __launch_bounds__(BA_THREADS) void bias_act_bwd_reduce_kernel(
    const float* __restrict__ slab, float* __restrict__ db, uint32_t nblocks,
    uint32_t C) {
  __shared__ float red[BA_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid / BA_RCOLS;
  const uint32_t c = blockIdx.x * BA_RCOLS + tid % BA_RCOLS;
  float t = 0.f;
  if (c < C) {
    uint32_t b = lane;
    for (; b + 3 * BA_RLANES < nblocks; b += 4 * BA_RLANES) {
      float a0 = slab[(size_t)b * C + c];
      float a1 = slab[(size_t)(b + BA_RLANES) * C + c];
      float a2 = slab[(size_t)(b + 2 * BA_RLANES) * C + c];
      float a3 = slab[(size_t)(b + 3 * BA_RLANES) * C + c];
      t += a0;
      t += a1;
      t += a2;
      t += a3;
    }
    for (; b < nblocks; b += BA_RLANES) t += slab[(size_t)b * C + c];
  }
  red[tid] = t;
  ba_barrier();
  if (lane == 0 && c < C) {
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < BA_RLANES; ++l) s += red[l * BA_RCOLS + tid];
    db[c] = s;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ============================================================== host side ==

static void ba_check_operand(const char* name, const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 ||
                              t.scalar_type() == at::kHalf),
              "bias_act_bwd: ", name, " must be a GPU bfloat16/float16 tensor");
  TORCH_CHECK((t.dim() == 2 && t.is_contiguous()) ||
                  (t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast)),
              "bias_act_bwd: ", name,
              " must be dense: contiguous 2-D or channels_last 4-D");
  TORCH_CHECK(t.numel() > 0 && t.numel() < (1ll << 31), "bias_act_bwd: ", name,
              " needs 0 < numel < 2^31, got ", t.numel());
  TORCH_CHECK(t.size(1) % 8 == 0, "bias_act_bwd: C % 8 == 0 required, got C = ",
              t.size(1));
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, "bias_act_bwd: ", name,
              " must be 16-byte aligned");
}

// (g, db32). relu = false: y is neither checked nor read, g is dy itself.
std::vector<at::Tensor> bias_act_bwd(const at::Tensor& dy, const at::Tensor& y,
                                     bool relu) {
  ba_check_operand("dy", dy);
  if (relu) {
    ba_check_operand("y", y);
    TORCH_CHECK(y.scalar_type() == dy.scalar_type() && y.device() == dy.device(),
                "bias_act_bwd: dy and y must have one dtype and one device");
    bool same = y.sizes() == dy.sizes();
    for (int64_t i = 0; same && i < dy.dim(); ++i)  // a size-1 dim addresses nothing
      same = dy.size(i) == 1 || y.stride(i) == dy.stride(i);
    TORCH_CHECK(same,
                "bias_act_bwd: dy and y must have the same sizes and strides");
  }
  const uint32_t C = dy.size(1), cvecs = C / 8;
  const uint32_t rows = (uint32_t)(dy.numel() / C);
  uint32_t bc, lanes, gy;
  if (cvecs <= (uint32_t)BA_THREADS) {
    bc = cvecs; lanes = BA_THREADS / bc; gy = 1;
  } else {
    bc = 64; lanes = BA_THREADS / 64; gy = (cvecs + 63) / 64;
  }
  const uint32_t walkers =
      std::min<uint32_t>((rows + lanes - 1) / lanes, BA_WALKERS);
  auto g = relu ? at::empty_like(dy) : dy;
  auto slab = at::empty({(long)walkers, (long)C}, dy.options().dtype(at::kFloat));
  auto db = at::empty({(long)C}, dy.options().dtype(at::kFloat));
  hipStream_t s = at::hip::getCurrentHIPStream().stream();
  const dim3 grid(walkers, gy);
  DTMX_DISPATCH_16(dy.scalar_type(), "bias_act_bwd", {
    if (relu)
      bias_act_bwd_kernel<elem_t, true><<<grid, BA_THREADS, 0, s>>>(
          (const elem_t*)dy.data_ptr(), (const elem_t*)y.data_ptr(),
          (elem_t*)g.data_ptr(), slab.data_ptr<float>(), rows, cvecs, bc, lanes);
    else
      bias_act_bwd_kernel<elem_t, false><<<grid, BA_THREADS, 0, s>>>(
          (const elem_t*)dy.data_ptr(), nullptr, nullptr,
          slab.data_ptr<float>(), rows, cvecs, bc, lanes);
  });
  bias_act_bwd_reduce_kernel<<<(C + BA_RCOLS - 1) / BA_RCOLS, BA_THREADS, 0, s>>>(
      slab.data_ptr<float>(), db.data_ptr<float>(), walkers, C);
  return {g, db};
}

}  // namespace dtmx
