// Native data pipeline: RecordIO parsing + JPEG decode + augmentation +
// threaded batch prefetch (reference: dmlc-core RecordIO +
// src/io/iter_image_recordio_2.cc:75-525 decode/augment threads +
// src/io/image_aug_default.cc resize/rand-crop/mirror augmenters — OpenCV
// replaced by libjpeg + a small bilinear resampler). Records carry either
// JPEG payloads (FFD8 magic; dims from the decoder) or raw uint8 HWC of
// exactly the target shape (the synthetic-bench fast path).
//
// On-disk format (dmlc RecordIO):
//   uint32 kMagic = 0xced7230a
//   uint32 lrec   = (cflag << 29) | length      (cflag 0 = whole record)
//   payload[length], padded to 4-byte alignment
// image records (reference image_recordio.h IRHeader):
//   uint32 flag; float label; uint64 id; uint64 id2;  then raw payload
#include <torch/extension.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <random>
#include <condition_variable>
#include <csetjmp>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <mutex>
#include <optional>
#include <thread>
#include <vector>

#include <jpeglib.h>

namespace dtmx {

// ------------------------------------------------------------ image helpers

struct Image {
  std::vector<uint8_t> pix;  // HWC
  int h = 0, w = 0, c = 0;
};

struct JpegErr {
  jpeg_error_mgr pub;
  jmp_buf jb;
};

static void jpeg_err_exit(j_common_ptr cinfo) {
  longjmp(((JpegErr*)cinfo->err)->jb, 1);
}

static bool is_jpeg(const uint8_t* p, size_t len) {
  return len >= 3 && p[0] == 0xFF && p[1] == 0xD8 && p[2] == 0xFF;
}

static bool decode_jpeg(const uint8_t* buf, size_t len, int want_c, Image& im) {
  jpeg_decompress_struct cinfo;
  JpegErr err;
  cinfo.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = jpeg_err_exit;
  if (setjmp(err.jb)) {
    jpeg_destroy_decompress(&cinfo);
    return false;
  }
  jpeg_create_decompress(&cinfo);
  jpeg_mem_src(&cinfo, const_cast<unsigned char*>(buf), len);
  jpeg_read_header(&cinfo, TRUE);
  cinfo.out_color_space = want_c == 1 ? JCS_GRAYSCALE : JCS_RGB;
  jpeg_start_decompress(&cinfo);
  im.h = cinfo.output_height;
  im.w = cinfo.output_width;
  im.c = cinfo.output_components;
  im.pix.resize((size_t)im.h * im.w * im.c);
  while (cinfo.output_scanline < cinfo.output_height) {
    uint8_t* row = im.pix.data() + (size_t)cinfo.output_scanline * im.w * im.c;
    jpeg_read_scanlines(&cinfo, &row, 1);
  }
  jpeg_finish_decompress(&cinfo);
  jpeg_destroy_decompress(&cinfo);
  return true;
}

static std::string encode_jpeg_impl(const uint8_t* pix, int h, int w, int c,
                                    int quality) {
  jpeg_compress_struct cinfo;
  JpegErr err;
  cinfo.err = jpeg_std_error(&err.pub);
  err.pub.error_exit = jpeg_err_exit;
  unsigned char* out = nullptr;
  unsigned long out_len = 0;
  if (setjmp(err.jb)) {
    jpeg_destroy_compress(&cinfo);
    if (out) free(out);
    return {};
  }
  jpeg_create_compress(&cinfo);
  jpeg_mem_dest(&cinfo, &out, &out_len);
  cinfo.image_width = w;
  cinfo.image_height = h;
  cinfo.input_components = c;
  cinfo.in_color_space = c == 1 ? JCS_GRAYSCALE : JCS_RGB;
  jpeg_set_defaults(&cinfo);
  jpeg_set_quality(&cinfo, quality, TRUE);
  jpeg_start_compress(&cinfo, TRUE);
  while (cinfo.next_scanline < cinfo.image_height) {
    JSAMPROW row = const_cast<uint8_t*>(pix + (size_t)cinfo.next_scanline * w * c);
    jpeg_write_scanlines(&cinfo, &row, 1);
  }
  jpeg_finish_compress(&cinfo);
  std::string s((const char*)out, out_len);
  jpeg_destroy_compress(&cinfo);
  free(out);
  return s;
}

// bilinear HWC uint8 resize (reference augmenter resize via cv::resize)
static Image resize_bilinear(const Image& src, int nh, int nw) {
  Image dst;
  dst.h = nh;
  dst.w = nw;
  dst.c = src.c;
  dst.pix.resize((size_t)nh * nw * src.c);
  const float sy = (float)src.h / nh, sx = (float)src.w / nw;
  for (int y = 0; y < nh; ++y) {
    float fy = (y + 0.5f) * sy - 0.5f;
    int y0 = std::max(0, (int)fy);
    int y1 = std::min(src.h - 1, y0 + 1);
    float wy = fy - y0;
    if (fy < 0) { y0 = y1 = 0; wy = 0.f; }
    for (int x = 0; x < nw; ++x) {
      float fx = (x + 0.5f) * sx - 0.5f;
      int x0 = std::max(0, (int)fx);
      int x1 = std::min(src.w - 1, x0 + 1);
      float wx = fx - x0;
      if (fx < 0) { x0 = x1 = 0; wx = 0.f; }
      for (int ch = 0; ch < src.c; ++ch) {
        float v00 = src.pix[((size_t)y0 * src.w + x0) * src.c + ch];
        float v01 = src.pix[((size_t)y0 * src.w + x1) * src.c + ch];
        float v10 = src.pix[((size_t)y1 * src.w + x0) * src.c + ch];
        float v11 = src.pix[((size_t)y1 * src.w + x1) * src.c + ch];
        float v = v00 * (1 - wy) * (1 - wx) + v01 * (1 - wy) * wx +
                  v10 * wy * (1 - wx) + v11 * wy * wx;
        dst.pix[((size_t)y * nw + x) * src.c + ch] = (uint8_t)(v + 0.5f);
      }
    }
  }
  return dst;
}

static constexpr uint32_t kRecMagic = 0xced7230a;

struct IRHeader {
  uint32_t flag;
  float label;
  uint64_t id;
  uint64_t id2;
};

class RecordIOReader {
 public:
  explicit RecordIOReader(const std::string& path) : path_(path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    TORCH_CHECK(f.good(), "cannot open ", path);
    size_t size = f.tellg();
    buf_.resize(size);
    f.seekg(0);
    f.read(buf_.data(), size);
    // index all records
    size_t pos = 0;
    while (pos + 8 <= buf_.size()) {
      uint32_t magic, lrec;
      std::memcpy(&magic, buf_.data() + pos, 4);
      std::memcpy(&lrec, buf_.data() + pos + 4, 4);
      TORCH_CHECK(magic == kRecMagic, "bad recordio magic at ", pos);
      uint32_t len = lrec & ((1u << 29) - 1);
      offsets_.emplace_back(pos + 8, len);
      pos += 8 + ((len + 3u) & ~3u);
    }
  }

  size_t size() const { return offsets_.size(); }

  std::pair<const char*, uint32_t> record(size_t i) const {
    auto [off, len] = offsets_.at(i);
    return {buf_.data() + off, len};
  }

  py::bytes read(size_t i) const {
    auto [p, len] = record(i);
    return py::bytes(p, len);
  }

 private:
  std::string path_;
  std::vector<char> buf_;
  std::vector<std::pair<size_t, uint32_t>> offsets_;
};

// ------------------------------------------------------ augmentation planner
//
// The staged loader's workers do no per-pixel work: they decode, and plan.
// A plan is the kAugPar-float row augment.hip documents (affine map, clamp
// box, fill, colour alphas + order, PCA add); every geometric step of the
// reference chain (image_aug_default.cc: resize, pad, the three crop
// branches; the iterator's mirror) is composed into the one affine map.
//
// Draws come from the per-record mt19937 in this fixed order, so a row
// depends on (seed, epoch, record, H, W) alone:
//   1. crop — random_resized_crop: per attempt (at most 10) area, aspect
//      ratio, swap coin; on the accepted attempt origin y, origin x.
//      min/max_crop_size: size; with rand_crop origin y, origin x.
//      otherwise, with rand_crop: origin y, origin x.
//   2. rand_mirror: one draw, low bit
//   3. brightness / contrast / saturation, if any is > 0: alpha_b, alpha_c,
//      alpha_s, order
//   4. pca_noise > 0: three normals (Box-Muller, two draws each)
// uniform = (draw >> 8) * 2^-24 in [0, 1); integer in [0, n) = draw % n.

static constexpr int kAugPar = 20;

struct AugConfig {
  int64_t th = 0, tw = 0;
  int64_t resize = 0, pad = 0;
  int64_t min_crop_size = -1, max_crop_size = -1;
  bool rand_crop = false, rand_mirror = false, random_resized_crop = false;
  double fill_value = 255;
  double min_random_area = 1, max_random_area = 1;
  double min_aspect_ratio = -1;  // < 0: unset, the range is 1 -+ max_aspect_ratio
  double max_aspect_ratio = 0;
  double brightness = 0, contrast = 0, saturation = 0, pca_noise = 0;
};

static AugConfig aug_config_from_dict(const py::dict& d) {
  AugConfig c;
  for (auto kv : d) {
    std::string k = py::cast<std::string>(kv.first);
    py::handle v = kv.second;
    if (k == "th") c.th = py::cast<int64_t>(v);
    else if (k == "tw") c.tw = py::cast<int64_t>(v);
    else if (k == "resize") c.resize = py::cast<int64_t>(v);
    else if (k == "pad") c.pad = py::cast<int64_t>(v);
    else if (k == "min_crop_size") c.min_crop_size = py::cast<int64_t>(v);
    else if (k == "max_crop_size") c.max_crop_size = py::cast<int64_t>(v);
    else if (k == "rand_crop") c.rand_crop = py::cast<bool>(v);
    else if (k == "rand_mirror") c.rand_mirror = py::cast<bool>(v);
    else if (k == "random_resized_crop") c.random_resized_crop = py::cast<bool>(v);
    else if (k == "fill_value") c.fill_value = py::cast<double>(v);
    else if (k == "min_random_area") c.min_random_area = py::cast<double>(v);
    else if (k == "max_random_area") c.max_random_area = py::cast<double>(v);
    else if (k == "min_aspect_ratio") c.min_aspect_ratio = py::cast<double>(v);
    else if (k == "max_aspect_ratio") c.max_aspect_ratio = py::cast<double>(v);
    else if (k == "brightness") c.brightness = py::cast<double>(v);
    else if (k == "contrast") c.contrast = py::cast<double>(v);
    else if (k == "saturation") c.saturation = py::cast<double>(v);
    else if (k == "pca_noise") c.pca_noise = py::cast<double>(v);
    else TORCH_CHECK(false, "augmentation config: unknown key '", k, "'");
  }
  TORCH_CHECK(c.th >= 1 && c.tw >= 1, "augmentation config: th and tw must be >= 1");
  TORCH_CHECK(c.resize >= 0 && c.pad >= 0, "augmentation config: resize and pad must be >= 0");
  return c;
}

struct AugRng {
  std::mt19937 g;
  float u01() { return (float)(g() >> 8) * (1.f / 16777216.f); }
  double uniform(double lo, double hi) { return lo + (hi - lo) * (double)u01(); }
  int64_t below(int64_t n) {  // always one draw
    uint32_t r = g();
    return n > 1 ? (int64_t)(r % (uint64_t)n) : 0;
  }
  double normal() {
    double u1 = 1.0 - (double)u01(), u2 = (double)u01();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
  }
};

static void aug_plan_row(const AugConfig& c, uint64_t seed, int64_t epoch,
                         size_t record, int64_t H, int64_t W, float* par) {
  AugRng rng{std::mt19937((uint32_t)(seed * 2654435761u + epoch * 97 + record))};
  // canvas (the reference's `res`) of Hc x Wc; canvas coordinate uc maps to
  // source coordinate uc * kx + ox (pixel edges at integers)
  double kx = 1, ky = 1, ox = 0, oy = 0;
  int64_t Hc = H, Wc = W;
  auto resize_to = [&](int64_t nh, int64_t nw) {
    nh = std::max<int64_t>(1, nh);
    nw = std::max<int64_t>(1, nw);
    kx *= (double)Wc / nw;
    ky *= (double)Hc / nh;
    Hc = nh;
    Wc = nw;
  };
  if (c.resize > 0) {  // shorter side, the reference's integer formula
    if (Hc > Wc) resize_to(c.resize * Hc / Wc, c.resize);
    else resize_to(c.resize, c.resize * Wc / Hc);
  }
  if (c.pad > 0) {
    ox -= c.pad * kx;
    oy -= c.pad * ky;
    Hc += 2 * c.pad;
    Wc += 2 * c.pad;
  }
  double min_ar = c.min_aspect_ratio, max_ar = c.max_aspect_ratio;
  if (min_ar < 0) {
    min_ar = 1 - c.max_aspect_ratio;
    max_ar = 1 + c.max_aspect_ratio;
  }
  int64_t cx = 0, cy = 0, cw = 0, ch = 0;
  bool cropped = false;
  if (c.random_resized_crop) {
    if (c.min_random_area != 1 || c.max_random_area != 1 || min_ar != 1 || max_ar != 1) {
      const double area = (double)Hc * Wc;
      for (int i = 0; i < 10 && !cropped; ++i) {
        double target = area * rng.uniform(c.min_random_area, c.max_random_area);
        double ratio = rng.uniform(min_ar, max_ar);
        int64_t h = (int64_t)std::llround(std::sqrt(target / ratio));
        int64_t w = (int64_t)std::llround(std::sqrt(target * ratio));
        if (rng.u01() > 0.5f) std::swap(h, w);
        if (h >= 1 && w >= 1 && h <= Hc && w <= Wc) {
          cy = rng.below(Hc - h + 1);
          cx = rng.below(Wc - w + 1);
          ch = h;
          cw = w;
          cropped = true;
        }
      }
    }
  } else if (c.min_crop_size != -1 || c.max_crop_size != -1) {
    // a size past the canvas is cut to it (the reference aborts there)
    int64_t s = c.min_crop_size + rng.below(c.max_crop_size - c.min_crop_size + 1);
    s = std::max<int64_t>(1, std::min(s, std::min(Hc, Wc)));
    if (c.rand_crop) {
      cy = rng.below(Hc - s + 1);
      cx = rng.below(Wc - s + 1);
    } else {
      cy = (Hc - s) / 2;
      cx = (Wc - s) / 2;
    }
    cw = ch = s;
    cropped = true;
  }
  if (!cropped) {
    // TH x TW window; a smaller canvas is first scaled up, aspect kept
    if (Hc < c.th)
      resize_to(c.th, (int64_t)((float)c.th / (float)Hc * (float)Wc));
    if (Wc < c.tw)
      resize_to((int64_t)((float)c.tw / (float)Wc * (float)Hc), c.tw);
    if (Hc < c.th) resize_to(c.th, Wc);  // float truncation left a row short
    if (c.rand_crop) {
      cy = rng.below(Hc - c.th + 1);
      cx = rng.below(Wc - c.tw + 1);
    } else {
      cy = (Hc - c.th) / 2;
      cx = (Wc - c.tw) / 2;
    }
    cw = c.tw;
    ch = c.th;
  }
  double a00 = kx * cw / c.tw, a02 = ox + cx * kx;
  double a11 = ky * ch / c.th, a12 = oy + cy * ky;
  // the crop rectangle's pixel centres, as source tap coordinates; without
  // pad also the image's, so a resize replicates its edge as cv::resize does
  double fx_lo = ox + (cx + 0.5) * kx - 0.5, fx_hi = ox + (cx + cw - 0.5) * kx - 0.5;
  double fy_lo = oy + (cy + 0.5) * ky - 0.5, fy_hi = oy + (cy + ch - 0.5) * ky - 0.5;
  if (c.pad == 0) {
    fx_lo = std::max(fx_lo, 0.0);
    fx_hi = std::min(fx_hi, (double)(W - 1));
    fy_lo = std::max(fy_lo, 0.0);
    fy_hi = std::min(fy_hi, (double)(H - 1));
  }
  if (c.rand_mirror && (rng.g() & 1)) {
    a02 += a00 * c.tw;
    a00 = -a00;
  }
  for (int i = 0; i < kAugPar; ++i) par[i] = 0.f;
  par[0] = (float)a00; par[2] = (float)a02;
  par[4] = (float)a11; par[5] = (float)a12;
  par[6] = (float)fx_lo; par[7] = (float)fx_hi;
  par[8] = (float)fy_lo; par[9] = (float)fy_hi;
  par[10] = (float)c.fill_value;
  par[11] = par[12] = par[13] = 1.f;
  if (c.brightness > 0 || c.contrast > 0 || c.saturation > 0) {
    par[11] = (float)(1.0 + rng.uniform(-c.brightness, c.brightness));
    par[12] = (float)(1.0 + rng.uniform(-c.contrast, c.contrast));
    par[13] = (float)(1.0 + rng.uniform(-c.saturation, c.saturation));
    par[14] = (float)rng.below(6);
  }
  if (c.pca_noise > 0) {
    // the published ImageNet RGB PCA (Krizhevsky et al. 2012): eigenvalue
    // times eigenvector, rows R, G, B
    static const double ev[3][3] = {
        {55.46 * -0.5675, 4.794 * 0.7192, 1.148 * 0.4009},
        {55.46 * -0.5808, 4.794 * -0.0045, 1.148 * -0.8140},
        {55.46 * -0.5836, 4.794 * -0.6948, 1.148 * 0.4203}};
    double al[3];
    for (int i = 0; i < 3; ++i) al[i] = c.pca_noise * rng.normal();
    for (int ch_ = 0; ch_ < 3; ++ch_)
      par[15 + ch_] = (float)(ev[ch_][0] * al[0] + ev[ch_][1] * al[1] + ev[ch_][2] * al[2]);
  }
}

// Threaded batch loader: worker threads unpack raw-uint8 image records into
// pinned float batches; a bounded queue feeds the Python iterator
// (reference PrefetcherIter/BatchLoader pipeline, src/io/iter_prefetcher.h).
class RecordBatchLoader {
 public:
  RecordBatchLoader(std::shared_ptr<RecordIOReader> reader, int64_t batch_size,
                    std::vector<int64_t> data_shape, int64_t part_index,
                    int64_t num_parts, bool shuffle, int64_t num_threads,
                    int64_t queue_capacity, int64_t seed,
                    bool rand_crop = false, bool rand_mirror = false,
                    int64_t resize = 0, std::optional<AugConfig> staged = {},
                    bool pin = false)
      : reader_(std::move(reader)),
        batch_(batch_size),
        shape_(std::move(data_shape)),
        shuffle_(shuffle),
        capacity_(std::max<int64_t>(1, queue_capacity)),
        rand_crop_(rand_crop),
        rand_mirror_(rand_mirror),
        resize_(resize),
        staged_(std::move(staged)),
        pin_(pin) {
    // shard records (reference part_index/num_parts sharding)
    size_t n = reader_->size();
    size_t per = n / num_parts;
    size_t start = part_index * per;
    size_t end = (part_index == num_parts - 1) ? n : start + per;
    for (size_t i = start; i < end; ++i) order_.push_back(i);
    rng_seed_ = seed;
    elem_ = 1;
    for (auto d : shape_) elem_ *= d;
    reset();
    for (int64_t t = 0; t < std::max<int64_t>(1, num_threads); ++t)
      workers_.emplace_back([this] { worker(); });
  }

  ~RecordBatchLoader() {
    {
      // under the lock: a worker between its predicate check and its wait
      // would otherwise miss the wake-up and never be joined
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_space_.notify_all();
    cv_item_.notify_all();
    for (auto& w : workers_) w.join();
  }

  void reset() {
    std::lock_guard<std::mutex> lk(mu_);
    if (shuffle_) {
      std::mt19937_64 rng(rng_seed_ + epoch_);
      std::shuffle(order_.begin(), order_.end(), rng);
    }
    cursor_ = 0;
    next_emit_ = 0;
    epoch_++;
    ready_.clear();
    cv_space_.notify_all();
  }

  int64_t batches_per_epoch() const { return order_.size() / batch_; }

  // returns (data[B,*shape] float32, label[B] float32) or empty tensors at
  // epoch end
  // Batches are delivered IN ORDER (batch k of the epoch's shuffled order is
  // the k-th item) regardless of worker completion order — matching the
  // reference's ordered threadediter semantics (dmlc threadediter.h).
  std::vector<at::Tensor> next() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_item_.wait(lk, [this] {
      return stop_ || ready_.count(next_emit_) ||
             next_emit_ >= batches_per_epoch();
    });
    auto it = ready_.find(next_emit_);
    if (it == ready_.end()) return {};
    auto out = std::move(it->second);
    ready_.erase(it);
    next_emit_++;
    cv_space_.notify_all();
    return out;
  }

 private:
  void worker() {
    while (!stop_) {
      int64_t b = -1, seq = 0;
      int64_t claim_epoch;
      {
        std::unique_lock<std::mutex> lk(mu_);
        // claim-gating bounds outstanding batches to the queue capacity so
        // the in-order reorder buffer can never deadlock on a slow worker
        cv_space_.wait(lk, [this] {
          return stop_ || cursor_ + batch_ > (int64_t)order_.size() ||
                 cursor_ / batch_ < next_emit_ + capacity_;
        });
        if (stop_) return;
        claim_epoch = epoch_;
        if (cursor_ + batch_ <= (int64_t)order_.size() &&
            cursor_ / batch_ < next_emit_ + capacity_) {
          b = cursor_;
          seq = b / batch_;
          cursor_ += batch_;
        }
      }
      if (b < 0) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        continue;
      }
      if (staged_) {
        auto out = stage_batch(b, claim_epoch);
        std::lock_guard<std::mutex> lk(mu_);
        if (epoch_ != claim_epoch) continue;
        ready_[seq] = std::move(out);
        cv_item_.notify_all();
        continue;
      }
      auto data = at::empty({batch_, shape_[0], shape_[1], shape_[2]},
                            at::kFloat);
      auto label = at::empty({batch_}, at::kFloat);
      float* dp = data.data_ptr<float>();
      float* lp = label.data_ptr<float>();
      const int TH = shape_[0], TW = shape_[1], TC = shape_[2];
      for (int64_t i = 0; i < batch_; ++i) {
        auto [p, len] = reader_->record(order_[b + i]);
        TORCH_CHECK(len > sizeof(IRHeader), "record too short");
        IRHeader h;
        std::memcpy(&h, p, sizeof(h));
        lp[i] = h.label;
        const uint8_t* raw = (const uint8_t*)(p + sizeof(IRHeader));
        size_t raw_len = len - sizeof(IRHeader);
        float* out = dp + i * elem_;
        // per-RECORD deterministic rng: augmentation is reproducible for a
        // given seed regardless of thread assignment (reference per-thread
        // kRandMagic seeds are scheduler-dependent — improved here)
        std::mt19937 rng((uint32_t)(rng_seed_ * 2654435761u +
                                    claim_epoch * 97 + order_[b + i]));
        if (is_jpeg(raw, raw_len) || rand_crop_ || rand_mirror_ || resize_) {
          Image im;
          if (is_jpeg(raw, raw_len)) {
            TORCH_CHECK(decode_jpeg(raw, raw_len, TC, im),
                        "JPEG decode failed for record ", order_[b + i]);
            TORCH_CHECK(im.c == TC, "record has ", im.c, " channels, want ", TC);
          } else {
            TORCH_CHECK((int64_t)raw_len >= elem_, "record too short");
            im.h = TH; im.w = TW; im.c = TC;
            im.pix.assign(raw, raw + elem_);
          }
          // resize shorter side (reference image_aug_default.cc resize aug)
          if (resize_ > 0) {
            int nh, nw;
            if (im.h < im.w) { nh = resize_; nw = (int)((int64_t)im.w * resize_ / im.h); }
            else { nw = resize_; nh = (int)((int64_t)im.h * resize_ / im.w); }
            if (nh != im.h || nw != im.w) im = resize_bilinear(im, nh, nw);
          }
          // crop to target (random or center); upscale if smaller
          if (im.h < TH || im.w < TW)
            im = resize_bilinear(im, std::max(im.h, TH), std::max(im.w, TW));
          int y0, x0;
          if (rand_crop_) {
            y0 = im.h == TH ? 0 : (int)(rng() % (im.h - TH + 1));
            x0 = im.w == TW ? 0 : (int)(rng() % (im.w - TW + 1));
          } else {
            y0 = (im.h - TH) / 2;
            x0 = (im.w - TW) / 2;
          }
          bool mirror = rand_mirror_ && (rng() & 1);
          for (int y = 0; y < TH; ++y)
            for (int x = 0; x < TW; ++x) {
              int sx = mirror ? (x0 + TW - 1 - x) : (x0 + x);
              const uint8_t* s = im.pix.data() +
                  (((size_t)(y0 + y)) * im.w + sx) * TC;
              float* o = out + ((size_t)y * TW + x) * TC;
              for (int ch = 0; ch < TC; ++ch) o[ch] = s[ch] * (1.f / 255.f);
            }
        } else {
          TORCH_CHECK((int64_t)raw_len >= elem_, "record too short");
          for (int64_t e = 0; e < elem_; ++e) out[e] = raw[e] * (1.f / 255.f);
        }
      }
      std::lock_guard<std::mutex> lk(mu_);
      if (epoch_ != claim_epoch) continue;  // reset() raced: drop stale batch
      ready_[seq] = {data, label};
      cv_item_.notify_all();
    }
  }

  // Staged mode: decode, plan, pack. Returns (src uint8[bytes] = the batch's
  // decoded RGB images back to back, geom int64[B][3] = {byte offset, H, W},
  // par float[B][kAugPar], label float[B]); all pinned when pin_ is set. A
  // raw record has the target shape, or the H x W its header's id2 field
  // names as (H << 32) | W when its payload is exactly H * W * 3 bytes
  // (tools/im2rec.py --raw-size writes such records).
  std::vector<at::Tensor> stage_batch(int64_t b, int64_t claim_epoch) {
    const AugConfig& cfg = *staged_;
    std::vector<Image> ims(batch_);
    std::vector<const uint8_t*> raws(batch_, nullptr);
    auto opt = [this](at::ScalarType t) {
      return at::TensorOptions().dtype(t).pinned_memory(pin_);
    };
    auto geom = at::empty({batch_, 3}, opt(at::kLong));
    auto par = at::empty({batch_, kAugPar}, opt(at::kFloat));
    auto label = at::empty({batch_}, opt(at::kFloat));
    int64_t* gp = geom.data_ptr<int64_t>();
    int64_t total = 0;
    for (int64_t i = 0; i < batch_; ++i) {
      auto [p, len] = reader_->record(order_[b + i]);
      TORCH_CHECK(len > sizeof(IRHeader), "record too short");
      IRHeader h;
      std::memcpy(&h, p, sizeof(h));
      label.data_ptr<float>()[i] = h.label;
      const uint8_t* raw = (const uint8_t*)(p + sizeof(IRHeader));
      size_t raw_len = len - sizeof(IRHeader);
      int64_t H, W;
      if (is_jpeg(raw, raw_len)) {
        TORCH_CHECK(decode_jpeg(raw, raw_len, 3, ims[i]),
                    "JPEG decode failed for record ", order_[b + i]);
        TORCH_CHECK(ims[i].c == 3, "record has ", ims[i].c, " channels, want 3");
        H = ims[i].h;
        W = ims[i].w;
      } else {
        // id2 counts as a size only when it accounts for the payload
        // exactly; H and W are bounded by raw_len before they are multiplied
        const int64_t n = (int64_t)raw_len;
        H = (int64_t)(h.id2 >> 32);
        W = (int64_t)(h.id2 & 0xffffffffu);
        if (!(H >= 1 && W >= 1 && H <= n && W <= n / H && H * W * 3 == n)) {
          H = cfg.th;
          W = cfg.tw;
        }
        TORCH_CHECK(n >= H * W * 3, "record too short");
        raws[i] = raw;
      }
      gp[i * 3] = total;
      gp[i * 3 + 1] = H;
      gp[i * 3 + 2] = W;
      total += H * W * 3;
      aug_plan_row(cfg, rng_seed_, claim_epoch, order_[b + i], H, W,
                   par.data_ptr<float>() + i * kAugPar);
    }
    auto src = at::empty({total}, opt(at::kByte));
    uint8_t* sp = src.data_ptr<uint8_t>();
    for (int64_t i = 0; i < batch_; ++i)
      std::memcpy(sp + gp[i * 3], raws[i] ? raws[i] : ims[i].pix.data(),
                  (size_t)(gp[i * 3 + 1] * gp[i * 3 + 2] * 3));
    return {src, geom, par, label};
  }

  std::shared_ptr<RecordIOReader> reader_;
  int64_t batch_;
  std::vector<int64_t> shape_;
  bool shuffle_;
  int64_t capacity_;
  bool rand_crop_ = false;
  bool rand_mirror_ = false;
  int64_t resize_ = 0;
  std::optional<AugConfig> staged_;
  bool pin_ = false;
  int64_t elem_ = 0;
  std::vector<size_t> order_;
  int64_t cursor_ = 0;
  int64_t next_emit_ = 0;
  int64_t epoch_ = 0;
  uint64_t rng_seed_ = 0;
  std::map<int64_t, std::vector<at::Tensor>> ready_;
  std::mutex mu_;
  std::condition_variable cv_item_, cv_space_;
  std::atomic<bool> stop_{false};
  std::vector<std::thread> workers_;
};

void write_recordio(const std::string& path, const std::vector<py::bytes>& records) {
  std::ofstream f(path, std::ios::binary);
  TORCH_CHECK(f.good(), "cannot open ", path);
  for (const auto& r : records) {
    std::string s = r;
    uint32_t magic = kRecMagic;
    uint32_t lrec = (uint32_t)s.size();
    f.write((const char*)&magic, 4);
    f.write((const char*)&lrec, 4);
    f.write(s.data(), s.size());
    static const char pad[4] = {0, 0, 0, 0};
    size_t p = (4 - (s.size() & 3)) & 3;
    f.write(pad, p);
  }
}

void register_recordio(py::module_& m) {
  py::class_<RecordIOReader, std::shared_ptr<RecordIOReader>>(m, "RecordIOReader")
      .def(py::init<const std::string&>())
      .def("__len__", &RecordIOReader::size)
      .def("read", &RecordIOReader::read);
  py::class_<RecordBatchLoader>(m, "RecordBatchLoader")
      .def(py::init<std::shared_ptr<RecordIOReader>, int64_t,
                    std::vector<int64_t>, int64_t, int64_t, bool, int64_t,
                    int64_t, int64_t, bool, bool, int64_t>(),
           py::arg("reader"), py::arg("batch_size"), py::arg("data_shape"),
           py::arg("part_index"), py::arg("num_parts"), py::arg("shuffle"),
           py::arg("num_threads"), py::arg("queue_capacity"), py::arg("seed"),
           py::arg("rand_crop") = false, py::arg("rand_mirror") = false,
           py::arg("resize") = 0)
      // staged mode: next() returns (src, geom, par, label) for augment_batch
      .def(py::init([](std::shared_ptr<RecordIOReader> reader, int64_t batch_size,
                       int64_t part_index, int64_t num_parts, bool shuffle,
                       int64_t num_threads, int64_t queue_capacity, int64_t seed,
                       const py::dict& aug, bool pin) {
             AugConfig cfg = aug_config_from_dict(aug);
             return new RecordBatchLoader(
                 std::move(reader), batch_size, {cfg.th, cfg.tw, 3}, part_index,
                 num_parts, shuffle, num_threads, queue_capacity, seed, false,
                 false, 0, cfg, pin);
           }),
           py::arg("reader"), py::arg("batch_size"), py::arg("part_index"),
           py::arg("num_parts"), py::arg("shuffle"), py::arg("num_threads"),
           py::arg("queue_capacity"), py::arg("seed"), py::arg("aug"),
           py::arg("pin") = false)
      .def("reset", &RecordBatchLoader::reset)
      .def("batches_per_epoch", &RecordBatchLoader::batches_per_epoch)
      .def("next", &RecordBatchLoader::next,
           py::call_guard<py::gil_scoped_release>());
  m.def("aug_plan",
        [](const py::dict& cfg, int64_t seed, int64_t epoch, int64_t record_id,
           int64_t H, int64_t W) {
          TORCH_CHECK(H >= 1 && W >= 1, "aug_plan: H and W must be >= 1");
          AugConfig c = aug_config_from_dict(cfg);
          auto row = at::empty({kAugPar}, at::kFloat);
          aug_plan_row(c, (uint64_t)seed, epoch, (size_t)record_id, H, W,
                       row.data_ptr<float>());
          return row;
        },
        py::arg("cfg"), py::arg("seed"), py::arg("epoch"), py::arg("record_id"),
        py::arg("H"), py::arg("W"));
  m.def("write_recordio", &write_recordio);
  m.def("encode_jpeg",
        [](py::bytes raw, int h, int w, int c, int quality) {
          std::string s = raw;
          TORCH_CHECK((int)s.size() >= h * w * c, "encode_jpeg: short buffer");
          auto out = encode_jpeg_impl((const uint8_t*)s.data(), h, w, c,
                                      quality);
          TORCH_CHECK(!out.empty(), "encode_jpeg failed");
          return py::bytes(out);
        },
        py::arg("raw"), py::arg("h"), py::arg("w"), py::arg("c"),
        py::arg("quality") = 95);
  m.def("decode_jpeg", [](py::bytes data, int want_c) {
    std::string s = data;
    Image im;
    TORCH_CHECK(decode_jpeg((const uint8_t*)s.data(), s.size(), want_c, im),
                "decode_jpeg failed");
    auto t = at::empty({im.h, im.w, im.c}, at::kByte);
    std::memcpy(t.data_ptr(), im.pix.data(), im.pix.size());
    return t;
  });
}

}  // namespace dtmx
