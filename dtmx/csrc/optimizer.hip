// Fused flat-bucket optimizer steps beyond plain SGD, for gfx950:
//
//   LBSGD  large-batch SGD with a layer-wise trust ratio (reference python
//          optimizer.py LBSGD): per-parameter ("segment") squared norms of the
//          fp32 master and the preprocessed gradient are reduced on the
//          device, turned into one learning rate per segment, and the
//          sgd_mom_mp update body runs with that rate. No host sync: the step
//          is hipGraph-capturable.
//   NAG    Nesterov momentum (reference optimizer_op-inl.h NAGMomKernel), flat
//          like sgd_mom_mp.
//
// A bucket's flat holds its parameters back to back; segment s is the element
// range [seg_off[s], seg_off[s+1]). The flat is cut into chunks of at most
// OPT_CHUNK consecutive elements of ONE segment, counted from the segment's
// start, so a parameter's reduction order depends on its own size only — not
// on its neighbours or its offset in the bucket. The chunk tables
// (dtmx/parallel/bucketer.py build_segment_tables) are device int32:
//   chunk_seg[c]      segment of chunk c
//   chunk_start[c]    first element of chunk c, as an index into the flat
//   chunk_len[c]      1..OPT_CHUNK
//   seg_chunk_off[s]  first chunk of segment s (nseg+1 entries)
// Segments start at any element offset, so every access is scalar (2-byte
// aligned is enough); a wave still reads 128 contiguous bytes per load.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "dtmx_common.h"

namespace dtmx {

#define OPT_CHUNK 4096
#define OPT_THREADS 256
#define OPT_MAX_BLOCKS 8192

static hipStream_t opt_stream() { return at::hip::getCurrentHIPStream().stream(); }

// hyper = {lr, momentum, wd, rescale, clip, eta}; the first five slots are
// those of sgd_mom_mp_dev.
struct OptHyper {
  float lr, momentum, wd, rescale, clip, eta;
};

template <bool DEV, bool ETA = true>
__device__ __forceinline__ OptHyper load_hyper(OptHyper h, const float* __restrict__ p) {
  if (DEV) {
    h.lr = p[0]; h.momentum = p[1]; h.wd = p[2];
    h.rescale = p[3]; h.clip = p[4];
    if (ETA) h.eta = p[5];
  }
  return h;
}

// ---- segment squared norms, stage 1: one block per chunk ------------------
// part[c] = {sum master^2, sum g^2}, g = clip(rescale * grad) BEFORE weight
// decay (the preprocessing of sgd_mom_mp_kernel). Fixed order: each thread
// sums its elements t, t+256, ... serially, then a 6-level shuffle tree per
// wave and a 2-level tree over the four wave sums through LDS. Every chunk's
// pair is stored, so the workspace needs no zero fill.
template <typename elem_t, bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void seg_sqnorm_part_kernel(
    const elem_t* __restrict__ g, const float* __restrict__ master,
    const int* __restrict__ chunk_start, const int* __restrict__ chunk_len,
    uint32_t nchunks, uint32_t total, float* __restrict__ part, OptHyper hy,
    const float* __restrict__ hyper) {
  const OptHyper h = load_hyper<DEV>(hy, hyper);
  const uint32_t t = threadIdx.x;
  __shared__ float red[2][OPT_THREADS / DTMX_WAVE];
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint32_t start = (uint32_t)chunk_start[c];
    uint32_t len = (uint32_t)chunk_len[c];
    if (start >= total) len = 0;                       // never leave the flat
    else if (len > total - start) len = total - start;
    const elem_t* gp = g + start;
    const float* mp = master + start;
    float sw = 0.f, sg = 0.f;
    for (uint32_t i = t; i < len; i += OPT_THREADS) {
      const float m = mp[i];
      float gv = (float)gp[i] * h.rescale;
      if (h.clip > 0.f) gv = fminf(fmaxf(gv, -h.clip), h.clip);
      sw += m * m;
      sg += gv * gv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sw += __shfl_down(sw, o);
      sg += __shfl_down(sg, o);
    }
    if ((t & 63) == 0) {
      red[0][t >> 6] = sw;
      red[1][t >> 6] = sg;
    }
    __syncthreads();
    if (t == 0) {
      part[2 * (size_t)c] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      part[2 * (size_t)c + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
    __syncthreads();  // red is reused by the next chunk of this block
  }
}

// ---- stage 2: one wave per segment ----------------------------------------
// fp64 sum of the segment's chunk partials in a fixed order (lane l takes
// chunks l, l+64, ... in turn, then a 6-level tree), then the segment's
// learning rate by the rule of LBSGD.update:
//   wn = sqrt(sq_w), gn = sqrt(sq_g); seg_lr = lr
//   if wn > 0 and gn > 0: seg_lr = min(lr * eta*wn / (gn + wd*wn + 1e-12), lr)
template <bool DEV>
__global__ __launch_bounds__(DTMX_WAVE) void seg_sqnorm_final_kernel(
    const float* __restrict__ part, const int* __restrict__ seg_chunk_off,
    uint32_t nchunks, double* __restrict__ sq, float* __restrict__ seg_lr,
    OptHyper hy, const float* __restrict__ hyper) {
  const OptHyper h = load_hyper<DEV>(hy, hyper);
  const uint32_t s = blockIdx.x, l = threadIdx.x;
  uint32_t c0 = (uint32_t)seg_chunk_off[s], c1 = (uint32_t)seg_chunk_off[s + 1];
  if (c1 > nchunks) c1 = nchunks;
  double sw = 0.0, sg = 0.0;
  for (uint32_t c = c0 + l; c < c1; c += DTMX_WAVE) {
    sw += (double)part[2 * (size_t)c];
    sg += (double)part[2 * (size_t)c + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sw += __shfl_down(sw, o);
    sg += __shfl_down(sg, o);
  }
  if (l == 0) {
    sq[2 * (size_t)s] = sw;
    sq[2 * (size_t)s + 1] = sg;
    const double lr = (double)h.lr, wn = sqrt(sw), gn = sqrt(sg);
    double r = lr;
    if (wn > 0.0 && gn > 0.0)
      r = fmin(lr * ((double)h.eta * wn / (gn + (double)h.wd * wn + 1e-12)), lr);
    seg_lr[s] = (float)r;
  }
}

// ---- LBSGD update: the body of sgd_mom_mp_kernel with lr = seg_lr[segment] -
template <typename elem_t, bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void lbsgd_mom_mp_kernel(
    elem_t* __restrict__ w, const elem_t* __restrict__ g,
    float* __restrict__ master, float* __restrict__ mom,
    const int* __restrict__ chunk_seg, const int* __restrict__ chunk_start,
    const int* __restrict__ chunk_len, const float* __restrict__ seg_lr,
    uint32_t nchunks, uint32_t nseg, uint32_t total, OptHyper hy,
    const float* __restrict__ hyper) {
  const OptHyper h = load_hyper<DEV>(hy, hyper);
  const float momentum = h.momentum, wd = h.wd, rescale = h.rescale, clip = h.clip;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint32_t s = (uint32_t)chunk_seg[c];
    const uint32_t start = (uint32_t)chunk_start[c];
    uint32_t len = (uint32_t)chunk_len[c];
    if (s >= nseg || start >= total) len = 0;          // never leave the flat
    else if (len > total - start) len = total - start;
    if (len == 0) continue;
    const float lr = seg_lr[s];
    for (uint32_t k = threadIdx.x; k < len; k += OPT_THREADS) {
      const size_t i = (size_t)start + k;
      float gv = (float)g[i] * rescale;
      if (clip > 0.f) gv = fminf(fmaxf(gv, -clip), clip);
      // Roundings spelled out as sgd_mom_mp_kernel is compiled (wd*master
      // fused into gv, the two products of the momentum line rounded
      // separately), so a segment running at lr is bit-equal to sgd_mom_mp;
      // left to the compiler, this loop contracts the momentum line.
      gv = __builtin_fmaf(wd, master[i], gv);
      float m;
      {
#pragma clang fp contract(off)
        m = momentum * mom[i] - lr * gv;
      }
      mom[i] = m;
      float nw = master[i] + m;
      master[i] = nw;
      w[i] = (elem_t)nw;
    }
  }
}

// ---- NAG, multi-precision ---------------------------------------------------
//   g32  = clip(grad * rescale) + wd * master
//   mom  = momentum * mom + g32
//   master -= lr * (g32 + momentum * mom);  w = bf16(master)
// momentum == 0 gives master -= lr * g32 (g32 + 0 * mom is g32 exactly).
template <typename elem_t, bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void nag_mom_mp_kernel(
    elem_t* __restrict__ w, const elem_t* __restrict__ g,
    float* __restrict__ master, float* __restrict__ mom, size_t total,
    OptHyper hy, const float* __restrict__ hyper) {
  const OptHyper h = load_hyper<DEV, false>(hy, hyper);  // five-entry buffers too
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    float gv = (float)g[i] * h.rescale;
    if (h.clip > 0.f) gv = fminf(fmaxf(gv, -h.clip), h.clip);
    gv += h.wd * master[i];
    float m = h.momentum * mom[i] + gv;
    mom[i] = m;
    // Not contracted: an fma that feeds the fp16 convert is folded into one
    // mixed-precision instruction that rounds once, and w would no longer be
    // the rounded fp32 master.
    float nw;
    {
#pragma clang fp contract(off)
      nw = master[i] - h.lr * (gv + h.momentum * m);
    }
    master[i] = nw;
    w[i] = (elem_t)nw;
  }
}

// ============================================================== host side ==

static void check_flats(const char* name, const at::Tensor& w16,
                        const at::Tensor& master, const at::Tensor* mom) {
  TORCH_CHECK(w16.is_cuda() && master.is_cuda(), name, ": flats must be on the GPU");
  TORCH_CHECK(w16.scalar_type() == at::kBFloat16 || w16.scalar_type() == at::kHalf,
              name, ": 16-bit flats must be bfloat16/float16");
  TORCH_CHECK(master.scalar_type() == at::kFloat, name, ": master must be float32");
  TORCH_CHECK(w16.dim() == 1 && master.dim() == 1 && w16.is_contiguous() &&
                  master.is_contiguous(),
              name, ": flats must be 1-D and contiguous");
  TORCH_CHECK(master.numel() == w16.numel(), name, ": flats differ in length (",
              w16.numel(), " vs master ", master.numel(), ")");
  TORCH_CHECK(master.device() == w16.device(), name, ": flats on different devices");
  TORCH_CHECK(w16.numel() < (int64_t(1) << 31), name, ": numel must be < 2^31");
  if (mom) {
    TORCH_CHECK(mom->is_cuda() && mom->scalar_type() == at::kFloat &&
                    mom->dim() == 1 && mom->is_contiguous(),
                name, ": mom must be a contiguous float32 GPU flat");
    TORCH_CHECK(mom->numel() == w16.numel(), name, ": flats differ in length (",
                w16.numel(), " vs mom ", mom->numel(), ")");
    TORCH_CHECK(mom->device() == w16.device(), name, ": flats on different devices");
  }
}

static void check_same16(const char* name, const at::Tensor& w, const at::Tensor& g) {
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == w.scalar_type(), name,
              ": grad must have the dtype of w");
  TORCH_CHECK(g.dim() == 1 && g.is_contiguous() && g.numel() == w.numel(), name,
              ": flats differ in length (", w.numel(), " vs grad ", g.numel(), ")");
  TORCH_CHECK(g.device() == w.device(), name, ": flats on different devices");
}

static void check_table(const char* name, const char* what, const at::Tensor& t,
                        const at::Tensor& like, int64_t n) {
  TORCH_CHECK(t.scalar_type() == at::kInt, name, ": ", what, " must be int32");
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, ": ", what,
              " must be on the device of the flats");
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous() && t.numel() == n, name, ": ",
              what, " must be contiguous with ", n, " entries, has ", t.numel());
}

// seg_off is the host (CPU int32) copy of the segment offsets, nseg+1 entries.
static int64_t check_seg_off(const char* name, const at::Tensor& seg_off,
                             int64_t numel) {
  TORCH_CHECK(!seg_off.is_cuda() && seg_off.scalar_type() == at::kInt &&
                  seg_off.dim() == 1 && seg_off.is_contiguous() &&
                  seg_off.numel() >= 1,
              name, ": seg_off must be a contiguous CPU int32 vector");
  const int* p = seg_off.data_ptr<int>();
  const int64_t n = seg_off.numel();
  TORCH_CHECK(p[0] == 0, name, ": seg_off must start at 0");
  for (int64_t i = 1; i < n; ++i)
    TORCH_CHECK(p[i] >= p[i - 1], name, ": seg_off must be non-decreasing (entry ",
                i, ")");
  TORCH_CHECK(p[n - 1] == numel, name, ": seg_off must end at numel (", p[n - 1],
              " vs ", numel, ")");
  return n - 1;
}

static void check_hyper(const char* name, const at::Tensor& hyper,
                        const at::Tensor& like, int64_t n) {
  TORCH_CHECK(hyper.is_cuda() && hyper.device() == like.device() &&
                  hyper.scalar_type() == at::kFloat && hyper.is_contiguous() &&
                  hyper.numel() >= n,
              name, ": hyper must be a float32 GPU buffer of >= ", n,
              " entries {lr, momentum, wd, rescale, clip, eta}");
}

static uint32_t chunk_grid(int64_t nchunks) {
  return (uint32_t)std::min<int64_t>(nchunks, OPT_MAX_BLOCKS);
}

int64_t opt_chunk() { return OPT_CHUNK; }

// stages: bit 0 = per-chunk partials, bit 1 = per-segment sums and seg_lr.
void seg_sqnorm(const at::Tensor& g, const at::Tensor& master,
                const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                const at::Tensor& seg_chunk_off, const at::Tensor& seg_off,
                at::Tensor part, at::Tensor sq, at::Tensor seg_lr, double lr,
                double wd, double rescale, double clip, double eta,
                const c10::optional<at::Tensor>& hyper, int64_t stages) {
  const char* name = "seg_sqnorm";
  check_flats(name, g, master, nullptr);
  const int64_t total = g.numel(), nchunks = chunk_start.numel();
  const int64_t nseg = check_seg_off(name, seg_off, total);
  check_table(name, "chunk_start", chunk_start, g, nchunks);
  check_table(name, "chunk_len", chunk_len, g, nchunks);
  check_table(name, "seg_chunk_off", seg_chunk_off, g, nseg + 1);
  TORCH_CHECK(part.is_cuda() && part.device() == g.device() &&
                  part.scalar_type() == at::kFloat && part.is_contiguous() &&
                  part.numel() == 2 * nchunks,
              name, ": part must be float32 [nchunks][2] on the device of the flats");
  TORCH_CHECK(sq.is_cuda() && sq.device() == g.device() &&
                  sq.scalar_type() == at::kDouble && sq.is_contiguous() &&
                  sq.numel() == 2 * nseg,
              name, ": sq must be float64 [nseg][2] on the device of the flats");
  TORCH_CHECK(seg_lr.is_cuda() && seg_lr.device() == g.device() &&
                  seg_lr.scalar_type() == at::kFloat && seg_lr.is_contiguous() &&
                  seg_lr.numel() == nseg,
              name, ": seg_lr must be float32 [nseg] on the device of the flats");
  TORCH_CHECK(stages >= 1 && stages <= 3, name, ": stages must be 1, 2 or 3");
  const float* hp = nullptr;
  if (hyper.has_value()) {
    check_hyper(name, *hyper, g, 6);
    hp = hyper->data_ptr<float>();
  }
  const OptHyper h{(float)lr, 0.f, (float)wd, (float)rescale, (float)clip, (float)eta};
  if ((stages & 1) && nchunks > 0) {
    DTMX_DISPATCH_16(g.scalar_type(), "seg_sqnorm", {
      if (hp)
        seg_sqnorm_part_kernel<elem_t, true>
            <<<chunk_grid(nchunks), OPT_THREADS, 0, opt_stream()>>>(
                (const elem_t*)g.data_ptr(), master.data_ptr<float>(),
                chunk_start.data_ptr<int>(), chunk_len.data_ptr<int>(),
                (uint32_t)nchunks, (uint32_t)total, part.data_ptr<float>(), h, hp);
      else
        seg_sqnorm_part_kernel<elem_t, false>
            <<<chunk_grid(nchunks), OPT_THREADS, 0, opt_stream()>>>(
                (const elem_t*)g.data_ptr(), master.data_ptr<float>(),
                chunk_start.data_ptr<int>(), chunk_len.data_ptr<int>(),
                (uint32_t)nchunks, (uint32_t)total, part.data_ptr<float>(), h, hp);
    });
  }
  if ((stages & 2) && nseg > 0) {
    if (hp)
      seg_sqnorm_final_kernel<true><<<(uint32_t)nseg, DTMX_WAVE, 0, opt_stream()>>>(
          part.data_ptr<float>(), seg_chunk_off.data_ptr<int>(), (uint32_t)nchunks,
          sq.data_ptr<double>(), seg_lr.data_ptr<float>(), h, hp);
    else
      seg_sqnorm_final_kernel<false><<<(uint32_t)nseg, DTMX_WAVE, 0, opt_stream()>>>(
          part.data_ptr<float>(), seg_chunk_off.data_ptr<int>(), (uint32_t)nchunks,
          sq.data_ptr<double>(), seg_lr.data_ptr<float>(), h, hp);
  }
}

static void lbsgd_launch(at::Tensor& w, const at::Tensor& g, at::Tensor& master,
                         at::Tensor& mom, const at::Tensor& chunk_seg,
                         const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                         const at::Tensor& seg_lr, const at::Tensor& seg_off,
                         OptHyper h, const at::Tensor* hyper, const char* name) {
  check_flats(name, w, master, &mom);
  check_same16(name, w, g);
  const int64_t total = w.numel(), nchunks = chunk_seg.numel();
  const int64_t nseg = check_seg_off(name, seg_off, total);
  check_table(name, "chunk_seg", chunk_seg, w, nchunks);
  check_table(name, "chunk_start", chunk_start, w, nchunks);
  check_table(name, "chunk_len", chunk_len, w, nchunks);
  TORCH_CHECK(seg_lr.is_cuda() && seg_lr.device() == w.device() &&
                  seg_lr.scalar_type() == at::kFloat && seg_lr.is_contiguous() &&
                  seg_lr.numel() == nseg,
              name, ": seg_lr must be float32 [nseg] on the device of the flats");
  const float* hp = nullptr;
  if (hyper) {
    check_hyper(name, *hyper, w, 6);
    hp = hyper->data_ptr<float>();
  }
  if (nchunks == 0) return;
  DTMX_DISPATCH_16(w.scalar_type(), name, {
    if (hp)
      lbsgd_mom_mp_kernel<elem_t, true>
          <<<chunk_grid(nchunks), OPT_THREADS, 0, opt_stream()>>>(
              (elem_t*)w.data_ptr(), (const elem_t*)g.data_ptr(),
              master.data_ptr<float>(), mom.data_ptr<float>(),
              chunk_seg.data_ptr<int>(), chunk_start.data_ptr<int>(),
              chunk_len.data_ptr<int>(), seg_lr.data_ptr<float>(),
              (uint32_t)nchunks, (uint32_t)nseg, (uint32_t)total, h, hp);
    else
      lbsgd_mom_mp_kernel<elem_t, false>
          <<<chunk_grid(nchunks), OPT_THREADS, 0, opt_stream()>>>(
              (elem_t*)w.data_ptr(), (const elem_t*)g.data_ptr(),
              master.data_ptr<float>(), mom.data_ptr<float>(),
              chunk_seg.data_ptr<int>(), chunk_start.data_ptr<int>(),
              chunk_len.data_ptr<int>(), seg_lr.data_ptr<float>(),
              (uint32_t)nchunks, (uint32_t)nseg, (uint32_t)total, h, hp);
  });
}

void lbsgd_mom_mp(at::Tensor w, const at::Tensor& g, at::Tensor master,
                  at::Tensor mom, const at::Tensor& chunk_seg,
                  const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                  const at::Tensor& seg_lr, const at::Tensor& seg_off,
                  double momentum, double wd, double rescale, double clip) {
  const OptHyper h{0.f, (float)momentum, (float)wd, (float)rescale, (float)clip, 0.f};
  lbsgd_launch(w, g, master, mom, chunk_seg, chunk_start, chunk_len, seg_lr,
               seg_off, h, nullptr, "lbsgd_mom_mp");
}

void lbsgd_mom_mp_dev(at::Tensor w, const at::Tensor& g, at::Tensor master,
                      at::Tensor mom, const at::Tensor& chunk_seg,
                      const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                      const at::Tensor& seg_lr, const at::Tensor& seg_off,
                      const at::Tensor& hyper) {
  lbsgd_launch(w, g, master, mom, chunk_seg, chunk_start, chunk_len, seg_lr,
               seg_off, OptHyper{}, &hyper, "lbsgd_mom_mp_dev");
}

static void nag_launch(at::Tensor& w, const at::Tensor& g, at::Tensor& master,
                       at::Tensor& mom, OptHyper h, const at::Tensor* hyper,
                       const char* name) {
  check_flats(name, w, master, &mom);
  check_same16(name, w, g);
  const float* hp = nullptr;
  if (hyper) {
    check_hyper(name, *hyper, w, 5);
    hp = hyper->data_ptr<float>();
  }
  const size_t total = w.numel();
  if (total == 0) return;
  const uint32_t blocks = std::min<size_t>((total + 255) / 256, 4096);
  DTMX_DISPATCH_16(w.scalar_type(), name, {
    if (hp)
      nag_mom_mp_kernel<elem_t, true><<<blocks, OPT_THREADS, 0, opt_stream()>>>(
          (elem_t*)w.data_ptr(), (const elem_t*)g.data_ptr(),
          master.data_ptr<float>(), mom.data_ptr<float>(), total, h, hp);
    else
      nag_mom_mp_kernel<elem_t, false><<<blocks, OPT_THREADS, 0, opt_stream()>>>(
          (elem_t*)w.data_ptr(), (const elem_t*)g.data_ptr(),
          master.data_ptr<float>(), mom.data_ptr<float>(), total, h, hp);
  });
}

void nag_mom_mp(at::Tensor w, const at::Tensor& g, at::Tensor master,
                at::Tensor mom, double lr, double momentum, double wd,
                double rescale, double clip) {
  const OptHyper h{(float)lr, (float)momentum, (float)wd, (float)rescale,
                   (float)clip, 0.f};
  nag_launch(w, g, master, mom, h, nullptr, "nag_mom_mp");
}

void nag_mom_mp_dev(at::Tensor w, const at::Tensor& g, at::Tensor master,
                    at::Tensor mom, const at::Tensor& hyper) {
  nag_launch(w, g, master, mom, OptHyper{}, &hyper, "nag_mom_mp_dev");
}

}  // namespace dtmx
