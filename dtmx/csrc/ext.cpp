// dtmx._C python bindings (torch extension).
#include <torch/extension.h>

namespace dtmx {
// gemm_conv.hip
at::Tensor linear_fwd(const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&);
at::Tensor linear_dgrad(const at::Tensor&, const at::Tensor&);
at::Tensor linear_wgrad(const at::Tensor&, const at::Tensor&);
at::Tensor conv_fwd(const at::Tensor&, const at::Tensor&, long, long);
at::Tensor conv_dgrad(const at::Tensor&, const at::Tensor&, long, long, long, long,
                      const c10::optional<at::Tensor>&);
at::Tensor conv_wgrad(const at::Tensor&, const at::Tensor&, long, long, long, long);
at::Tensor conv_wgrad_nt256(const at::Tensor&, const at::Tensor&, long, long, long,
                            long, long, bool);
std::tuple<bool, long, bool> wgrad_nt256_plan(long, long, long);
std::tuple<long, long, long, long, long> gemm_plan(long, long, long, long, bool);
std::tuple<bool, long> smallgrid_plan(long, long, long);
std::tuple<long, long, long, bool, long, long> wgrad_nt_plan(long, long, long);
at::Tensor conv_wgrad_acc32(const at::Tensor&, const at::Tensor&, long, long, long,
                            long, bool, long, bool);
std::vector<at::Tensor> conv_dgrad_bnfuse(const at::Tensor&, const at::Tensor&,
                                          long, long, long, long,
                                          const c10::optional<at::Tensor>&,
                                          const at::Tensor&, const at::Tensor&,
                                          const at::Tensor&, const at::Tensor&,
                                          const c10::optional<at::Tensor>&);
std::vector<std::tuple<long, long, double>> wgrad_ws_stats();
// dwconv.hip
at::Tensor dwconv_fwd(const at::Tensor&, const at::Tensor&, long, long);
at::Tensor dwconv_dgrad(const at::Tensor&, const at::Tensor&, long, long, long, long);
at::Tensor dwconv_wgrad(const at::Tensor&, const at::Tensor&, long, long);
// gconv.hip
at::Tensor gconv_fwd(const at::Tensor&, const at::Tensor&, long, long, long);
at::Tensor gconv_dgrad(const at::Tensor&, const at::Tensor&, long, long, long, long,
                       long);
at::Tensor gconv_wgrad(const at::Tensor&, const at::Tensor&, long, long, long, bool);
// avgpool.hip
at::Tensor avgpool_fwd(const at::Tensor&, long, long, long, bool);
at::Tensor avgpool_bwd(const at::Tensor&, long, long, long, long, long, bool);
// augment.hip
at::Tensor augment_batch(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, const at::Tensor&, long, long,
                         at::ScalarType, const at::Tensor&, const at::Tensor&);
// batchnorm.hip
std::vector<at::Tensor> bn_fwd_train(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, at::Tensor, at::Tensor,
                                     double, double, bool,
                                     const c10::optional<at::Tensor>&,
                                     const c10::optional<at::Tensor>&,
                                     const c10::optional<at::Tensor>&, bool);
std::vector<at::Tensor> conv_fwd_stats(const at::Tensor&, const at::Tensor&,
                                       long, long);
std::vector<at::Tensor> bn_local_sums(const at::Tensor&);
std::vector<at::Tensor> bn_fwd_presummed(const at::Tensor&, const at::Tensor&,
                                         const at::Tensor&, at::Tensor,
                                         at::Tensor, double, double, bool,
                                         const c10::optional<at::Tensor>&,
                                         const at::Tensor&, const at::Tensor&,
                                         long);
std::vector<at::Tensor> bn_bwd_sums(const at::Tensor&, const at::Tensor&,
                                    const at::Tensor&, const at::Tensor&,
                                    const at::Tensor&, bool);
std::vector<at::Tensor> bn_bwd_finalize_slabs(const at::Tensor&, const at::Tensor&,
                                              const at::Tensor&);
std::vector<at::Tensor> bn_bwd_dx_presummed(const at::Tensor&, const at::Tensor&,
                                            const at::Tensor&, const at::Tensor&,
                                            const at::Tensor&, const at::Tensor&,
                                            const at::Tensor&, const at::Tensor&,
                                            long, bool, bool,
                                            const c10::optional<at::Tensor>&);
at::Tensor bn_fwd_infer(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                        const at::Tensor&, const at::Tensor&, double, bool,
                        const c10::optional<at::Tensor>&);
std::vector<at::Tensor> bn_bwd(const at::Tensor&, const at::Tensor&,
                               const at::Tensor&, const at::Tensor&,
                               const at::Tensor&, bool, const at::Tensor&, bool,
                               const c10::optional<at::Tensor>&);
// pool_elem.hip
std::vector<at::Tensor> maxpool_fwd(const at::Tensor&, long, long, long);
at::Tensor maxpool_bwd(const at::Tensor&, const at::Tensor&, long, long, long,
                       long, long);
at::Tensor global_avgpool_fwd(const at::Tensor&);
at::Tensor global_avgpool_bwd(const at::Tensor&, long, long);
at::Tensor relu_fwd(const at::Tensor&);
at::Tensor relu_bwd(const at::Tensor&, const at::Tensor&);
at::Tensor add_relu_fwd(const at::Tensor&, const at::Tensor&);
// softmax_opt.hip
std::vector<at::Tensor> softmax_ce_fwd(const at::Tensor&, const at::Tensor&);
at::Tensor softmax_ce_bwd(const at::Tensor&, const at::Tensor&, const at::Tensor&);
void sgd_mom_mp(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor, double,
                double, double, double, double);
void sgd_mom_mp_dev(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor,
                    const at::Tensor&);
void sgd_mom_f32(at::Tensor, const at::Tensor&, at::Tensor, double, double,
                 double, double, double);
// optimizer.hip
int64_t opt_chunk();
void seg_sqnorm(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                const at::Tensor&, const at::Tensor&, const at::Tensor&,
                at::Tensor, at::Tensor, at::Tensor, double, double, double,
                double, double, const c10::optional<at::Tensor>&, int64_t);
void lbsgd_mom_mp(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor,
                  const at::Tensor&, const at::Tensor&, const at::Tensor&,
                  const at::Tensor&, const at::Tensor&, double, double, double,
                  double);
void lbsgd_mom_mp_dev(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor,
                      const at::Tensor&, const at::Tensor&, const at::Tensor&,
                      const at::Tensor&, const at::Tensor&, const at::Tensor&);
void nag_mom_mp(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor, double,
                double, double, double, double);
void nag_mom_mp_dev(at::Tensor, const at::Tensor&, at::Tensor, at::Tensor,
                    const at::Tensor&);
// dropout_ln.hip
std::vector<at::Tensor> dropout_fwd(const at::Tensor&, double, int64_t);
at::Tensor dropout_bwd(const at::Tensor&, const at::Tensor&, double);
std::vector<at::Tensor> layer_norm_fwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, double);
std::vector<at::Tensor> layer_norm_bwd(const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&, const at::Tensor&,
                                       const at::Tensor&);
// compress.hip
at::Tensor quantize_2bit(const at::Tensor&, at::Tensor, double);
at::Tensor dequantize_2bit(const at::Tensor&, long, double);
// gemm256.hip
at::Tensor gemm256_nt(const at::Tensor&, const at::Tensor&);
at::Tensor gemm256n_nt(const at::Tensor&, const at::Tensor&);
at::Tensor lrn_fwd(const at::Tensor&, double, double, double);
at::Tensor lrn_bwd(const at::Tensor&, const at::Tensor&, double, double, double);
// indexing.hip
at::Tensor take_fwd(const at::Tensor&, const at::Tensor&);
at::Tensor take_bwd(const at::Tensor&, const at::Tensor&, long);
// recordio.cpp
void register_recordio(py::module_& m);
}  // namespace dtmx

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("linear_fwd", &dtmx::linear_fwd);
  m.def("linear_dgrad", &dtmx::linear_dgrad);
  m.def("linear_wgrad", &dtmx::linear_wgrad);
  m.def("conv_fwd", &dtmx::conv_fwd);
  m.def("conv_fwd_stats", &dtmx::conv_fwd_stats);
  m.def("conv_dgrad", &dtmx::conv_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("H"), py::arg("W"),
        py::arg("acc") = c10::nullopt);
  m.def("conv_wgrad", &dtmx::conv_wgrad);
  // test/bench entry: always the 256² contraction-major kernel
  m.def("conv_wgrad_nt256", &dtmx::conv_wgrad_nt256, py::arg("x"),
        py::arg("dy"), py::arg("R"), py::arg("S"), py::arg("stride"),
        py::arg("pad"), py::arg("splitk"), py::arg("group"));
  // test entry: fp32 split-K sums before the 16-bit rounding
  m.def("conv_wgrad_acc32", &dtmx::conv_wgrad_acc32, py::arg("x"),
        py::arg("dy"), py::arg("R"), py::arg("S"), py::arg("stride"),
        py::arg("pad"), py::arg("nt256"), py::arg("splitk"), py::arg("group"));
  // (use, splitk, group) the routing picks for a (Ko, RSC, NPQ) wgrad
  m.def("wgrad_nt256_plan", &dtmx::wgrad_nt256_plan, py::arg("Ko"),
        py::arg("RSC"), py::arg("NPQ"));
  // Read-only routing plans (the launchers call the same functions):
  // gemm_plan -> (kernel, tiles_m, tiles_n, slices, K-tiles per slice) with
  // kernel 256 = gemm256f_kernel, 4 / 2 = gemm_tn_kernel<4> / <2>; lds_stage
  // is false for the fp32-atomic (split-K) epilogue.
  m.def("gemm_plan", &dtmx::gemm_plan, py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("splitk") = 1, py::arg("lds_stage") = true);
  // (taken, splitk) of the small-grid fp32-atomic detour of conv fwd/dgrad
  m.def("smallgrid_plan", &dtmx::smallgrid_plan, py::arg("M"), py::arg("N"),
        py::arg("K"));
  // (wm, nj, depth, grouped, slices, K-tiles per slice) of the gemm_nt_kernel
  // launch for a wgrad that wgrad_nt256_plan does not claim
  m.def("wgrad_nt_plan", &dtmx::wgrad_nt_plan, py::arg("Ko"), py::arg("RSC"),
        py::arg("NPQ"));
  m.def("dwconv_fwd", &dtmx::dwconv_fwd, py::arg("x"), py::arg("w"),
        py::arg("stride"), py::arg("pad"));
  m.def("dwconv_dgrad", &dtmx::dwconv_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("H"), py::arg("W"));
  m.def("dwconv_wgrad", &dtmx::dwconv_wgrad, py::arg("x"), py::arg("dy"),
        py::arg("stride"), py::arg("pad"));
  m.def("gconv_fwd", &dtmx::gconv_fwd, py::arg("x"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("groups"));
  m.def("gconv_dgrad", &dtmx::gconv_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("stride"), py::arg("pad"), py::arg("groups"), py::arg("H"),
        py::arg("W"));
  m.def("gconv_wgrad", &dtmx::gconv_wgrad, py::arg("x"), py::arg("dy"),
        py::arg("stride"), py::arg("pad"), py::arg("groups"),
        py::arg("w_channels_last") = false);
  m.def("conv_dgrad_bnfuse", &dtmx::conv_dgrad_bnfuse, py::arg("dy"),
        py::arg("w"), py::arg("stride"), py::arg("pad"), py::arg("H"),
        py::arg("W"), py::arg("acc"), py::arg("y"), py::arg("xin"),
        py::arg("mean"), py::arg("invstd"), py::arg("mask") = py::none());
  m.def("bn_bwd_finalize_slabs", &dtmx::bn_bwd_finalize_slabs);
  m.def("wgrad_ws_stats", &dtmx::wgrad_ws_stats);
  // want_mask appends a 4th output: the packed relu mask, uint8
  // [N*H*W][C/8], bit e of byte (row, cv) = !(y[row][cv*8+e] <= 0). The
  // backward entries take it as `mask` in place of their y operand.
  m.def("bn_fwd_train", &dtmx::bn_fwd_train, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("running_mean"), py::arg("running_var"),
        py::arg("momentum"), py::arg("eps"), py::arg("fuse_relu"),
        py::arg("residual"), py::arg("pre_psum"), py::arg("pre_psumsq"),
        py::arg("want_mask") = false);
  m.def("bn_fwd_infer", &dtmx::bn_fwd_infer);
  m.def("bn_bwd", &dtmx::bn_bwd, py::arg("x"), py::arg("dy"), py::arg("gamma"),
        py::arg("save_mean"), py::arg("save_invstd"), py::arg("fuse_relu"),
        py::arg("y"), py::arg("want_dres"), py::arg("mask") = py::none());
  m.def("bn_local_sums", &dtmx::bn_local_sums);
  m.def("bn_fwd_presummed", &dtmx::bn_fwd_presummed);
  m.def("bn_bwd_sums", &dtmx::bn_bwd_sums);
  m.def("bn_bwd_dx_presummed", &dtmx::bn_bwd_dx_presummed, py::arg("x"),
        py::arg("dy"), py::arg("y"), py::arg("save_mean"),
        py::arg("save_invstd"), py::arg("gamma"), py::arg("tdb"),
        py::arg("tdg"), py::arg("count"), py::arg("fuse_relu"),
        py::arg("want_dres"), py::arg("mask") = py::none());
  m.def("maxpool_fwd", &dtmx::maxpool_fwd);
  m.def("maxpool_bwd", &dtmx::maxpool_bwd);
  m.def("avgpool_fwd", &dtmx::avgpool_fwd, py::arg("x"), py::arg("kernel"),
        py::arg("stride"), py::arg("pad"), py::arg("count_include_pad"));
  m.def("avgpool_bwd", &dtmx::avgpool_bwd, py::arg("dy"), py::arg("H"),
        py::arg("W"), py::arg("kernel"), py::arg("stride"), py::arg("pad"),
        py::arg("count_include_pad"));
  // Decoded uint8 records -> normalised (B,3,TH,TW) channels_last batch; the
  // plan row layout is documented in augment.hip. geom / par are device
  // tensors, geom_host / par_host their CPU copies (validated on the host);
  // mean / std are 3-element CPU float32 tensors.
  m.def("augment_batch", &dtmx::augment_batch, py::arg("src"), py::arg("geom"),
        py::arg("par"), py::arg("mean"), py::arg("std"), py::arg("TH"),
        py::arg("TW"), py::arg("out_dtype"), py::arg("geom_host"),
        py::arg("par_host"));
  m.def("global_avgpool_fwd", &dtmx::global_avgpool_fwd);
  m.def("global_avgpool_bwd", &dtmx::global_avgpool_bwd);
  m.def("relu_fwd", &dtmx::relu_fwd);
  m.def("relu_bwd", &dtmx::relu_bwd);
  m.def("add_relu_fwd", &dtmx::add_relu_fwd);
  m.def("softmax_ce_fwd", &dtmx::softmax_ce_fwd);
  m.def("softmax_ce_bwd", &dtmx::softmax_ce_bwd);
  m.def("sgd_mom_mp", &dtmx::sgd_mom_mp);
  m.def("sgd_mom_mp_dev", &dtmx::sgd_mom_mp_dev);
  m.def("sgd_mom_f32", &dtmx::sgd_mom_f32);
  // Segment ("per-parameter") view of a flat bucket: chunk tables are device
  // int32, seg_off is their host copy (CPU int32, nseg+1 entries). seg_sqnorm
  // fills part [nchunks][2] f32, sq [nseg][2] f64 = {sum master^2, sum g^2}
  // and seg_lr [nseg] f32; stages 1 / 2 / 3 = partials / final / both. With
  // `hyper` (device f32 {lr, momentum, wd, rescale, clip, eta}) the scalar
  // arguments are ignored.
  m.def("opt_chunk", &dtmx::opt_chunk);
  m.def("seg_sqnorm", &dtmx::seg_sqnorm, py::arg("grad"), py::arg("master"),
        py::arg("chunk_start"), py::arg("chunk_len"), py::arg("seg_chunk_off"),
        py::arg("seg_off"), py::arg("part"), py::arg("sq"), py::arg("seg_lr"),
        py::arg("lr"), py::arg("wd"), py::arg("rescale"), py::arg("clip"),
        py::arg("eta"), py::arg("hyper") = py::none(), py::arg("stages") = 3);
  m.def("lbsgd_mom_mp", &dtmx::lbsgd_mom_mp, py::arg("w"), py::arg("grad"),
        py::arg("master"), py::arg("mom"), py::arg("chunk_seg"),
        py::arg("chunk_start"), py::arg("chunk_len"), py::arg("seg_lr"),
        py::arg("seg_off"), py::arg("momentum"), py::arg("wd"),
        py::arg("rescale"), py::arg("clip"));
  m.def("lbsgd_mom_mp_dev", &dtmx::lbsgd_mom_mp_dev, py::arg("w"),
        py::arg("grad"), py::arg("master"), py::arg("mom"), py::arg("chunk_seg"),
        py::arg("chunk_start"), py::arg("chunk_len"), py::arg("seg_lr"),
        py::arg("seg_off"), py::arg("hyper"));
  m.def("nag_mom_mp", &dtmx::nag_mom_mp);
  m.def("nag_mom_mp_dev", &dtmx::nag_mom_mp_dev);
  m.def("dropout_fwd", &dtmx::dropout_fwd);
  m.def("dropout_bwd", &dtmx::dropout_bwd);
  m.def("layer_norm_fwd", &dtmx::layer_norm_fwd);
  m.def("layer_norm_bwd", &dtmx::layer_norm_bwd);
  m.def("gemm256_nt", &dtmx::gemm256_nt);
  m.def("gemm256n_nt", &dtmx::gemm256n_nt);
  m.def("lrn_fwd", &dtmx::lrn_fwd);
  m.def("lrn_bwd", &dtmx::lrn_bwd);
  m.def("take_fwd", &dtmx::take_fwd);
  m.def("take_bwd", &dtmx::take_bwd);
  m.def("quantize_2bit", &dtmx::quantize_2bit);
  m.def("dequantize_2bit", &dtmx::dequantize_2bit);
  dtmx::register_recordio(m);
}
