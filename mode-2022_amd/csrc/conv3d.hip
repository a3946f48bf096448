// The C entries of the 3-D convolution family (3x3x3, pad 1: the regulariser of MODE's disparity stage) and their argument checks.
// Pure host code; the kernels, each with the host function that launches it (conv3d_internal.h), are in
//   conv3d_f32_fwd.hip          fp32 MFMA: pack_w3d, conv3d_kernel (stride 1 | 2, also the stride-1 input gradient), deconv3d_kernel
//   conv3d_f32_wgrad.hip        fp32 MFMA: conv3d_bwd_weight_kernel, _s2_kernel, _ring_kernel; reduce_gw3d (every weight gradient's partials)
//   conv3d_c1.hip               the single-output-channel layers (classifier heads)
//   conv3d_split.hip            split operands (bf16 x 3, fp16 x 2): stride-1 forward / input gradient, and the abs_max kernels
//   conv3d_split_s2.hip, conv3d_split_deconv.hip         ... stride-2 forward; transposed convolution (= the stride-2 input gradient)
//   conv3d_split_wgrad.hip, conv3d_split_wgrad_s2.hip    ... weight gradient at stride 1; at stride 2
#include "common.h"
#include "conv3d_internal.h"
#include "bn_internal.h"

namespace {

// One check for every entry: the size rule; then, for an entry of the split kernels, `split_ok` -- the layer and the 32-bit contracts
// of the kernel the entry launches (mode_conv3d_split_shape_supported, size_contracts.h); pointers last, and none needed for an empty
// batch: a shape beyond a limit is MODE_ERR_UNSUPPORTED whatever the pointers are.  `at` completes the shape in split_ok's message.
template <typename Pred>
int check_args(const void* a, const void* b, const void* c, const void* wp, int B, int Ci, int D, int H, int W, int Co, int stride,
               bool allow_s2, const char* who, Pred split_ok, const char* at = "") {
  MODE_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: non-positive size", who);
  MODE_REQUIRE(stride == 1 || (stride == 2 && allow_s2), MODE_ERR_UNSUPPORTED, "%s: stride %d not implemented", who, stride);
  MODE_REQUIRE((long long)std::max(Ci, 8) * D * H * W < (1ll << 31) && (long long)std::max(Co, 8) * D * H * W < (1ll << 31),
               MODE_ERR_UNSUPPORTED, "%s: a sample larger than 2^31 elements", who);
  MODE_REQUIRE(split_ok(), MODE_ERR_UNSUPPORTED, "%s: %d -> %d channels at %dx%dx%d%s: not covered by the split kernel, or beyond its "
               "32-bit offsets (mode_conv3d_split_shape_supported)", who, Ci, Co, D, H, W, at);
  if (B == 0) return MODE_OK;
  MODE_REQUIRE(a && b && c && wp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  return MODE_OK;
}

// an entry of the fp32 kernels
int check_conv_args(const void* a, const void* b, const void* c, const void* wp, int B, int Ci, int D, int H, int W, int Co,
                    int stride, const char* who, bool allow_s2 = false) {
  return check_args(a, b, c, wp, B, Ci, D, H, W, Co, stride, allow_s2, who, [] { return true; });
}

// an entry of the split kernels: the forward / input gradient / weight gradient `which` of the CONVOLUTION (Ci, Co, D, H, W, stride)
int check_split_args(const void* a, const void* b, const void* c, const void* wp, int B, int Ci, int D, int H, int W, int Co, int stride,
                     int which, const char* who) {
  return check_args(a, b, c, wp, B, Ci, D, H, W, Co, stride, true, who,
                    [&] { return mode_conv3d_split_shape_supported(Ci, Co, D, H, W, stride, which) == 1; },
                    stride == 2 ? ", stride 2" : ", stride 1");
}

// ... and of the split transposed convolution (Cin, D, H, W) -> (Cout, 2D, 2H, 2W): the stride-2 input gradient Cout -> Cin at 2D x 2H x 2W
int check_deconv_split_args(const void* a, const void* b, const void* c, const void* wp, int B, int Cin, int D, int H, int W, int Cout,
                            const char* who) {
  return check_args(a, b, c, wp, B, Cin, D, H, W, Cout, 1, false, who, [&] {
    return D < (1 << 30) && H < (1 << 30) && W < (1 << 30) && mode_conv3d_split_shape_supported(Cout, Cin, 2 * D, 2 * H, 2 * W, 2, 1) == 1;
  });
}

// The weight gradient of an empty batch is zero: written unless the call accumulates.
int empty_batch_gw(float* gw, int Ci, int Co, int accumulate, hipStream_t st, const char* who) {
  return accumulate ? MODE_OK : mode::zero_floats(gw, (size_t)Co * Ci * 27, st, who);
}

}  // namespace

extern "C" size_t mode_conv3d_wpack_bytes(int Ci, int Co) {
  if (Ci <= 0 || Co <= 0) return 0;
  const size_t f = mode::conv3d_f32_pack_floats(Ci, Co), b = mode::conv3d_f32_pack_floats(Co, Ci);  // forward, input gradient
  size_t n = (f > b ? f : b) + 32 * (size_t)mode::cdiv(Co > Ci ? Co : Ci, 32);  // + the folded BatchNorm shifts
  n = std::max(n, std::max(mode::conv3d_split_wpack_floats(Ci, Co), mode::conv3d_split_wpack_floats(Co, Ci)));
  n = std::max(n, mode::conv3d_s2_split_wpack_floats(Ci, Co));
  n = std::max(n, std::max(mode::deconv3d_split_wpack_floats(Ci, Co), mode::deconv3d_split_wpack_floats(Co, Ci)));
  return n * sizeof(float);
}

extern "C" int mode_conv3d_split_supported(int Ci, int Co, int stride, int which) {
  if (Ci <= 0 || Co <= 0) return 0;
  if (stride == 2) {  // forward: mode_conv3d_fwd_s2_split; input gradient: mode_conv3d_bwd_data_s2_split (even volumes); weight gradient:
                      // mode_conv3d_bwd_weight_s2_split (even volumes, W a multiple of 8; gy in blocks of 64 channels, x in blocks of 32)
    if (which == 0) return mode::conv3d_s2_split_supported(Ci, Co) ? 1 : 0;
    if (which == 2) return (Co % 64 == 0 && Ci % 32 == 0) ? 1 : 0;
    return (which == 1 && mode::deconv3d_split_supported(Co, Ci)) ? 1 : 0;
  }
  if (stride != 1) return 0;
  if (which == 2) return Co > 1;  // weight gradient: any channel counts (32 x 32 blocks, masked)
  return which == 1 ? mode::conv3d_split_supported(Co, Ci) : mode::conv3d_split_supported(Ci, Co);
}

// Host only, launches nothing: 1 exactly when the layer's channel counts are supported (mode_conv3d_split_supported) AND the volume is
// inside every 32-bit contract of the kernel that the corresponding split entry launches (size_contracts.h has the derivations).
// (Ci, Co, D, H, W, stride) describe the CONVOLUTION -- x (Ci, D, H, W) -> y (Co, D / stride, ...) -- whichever of its three GEMMs
// `which` asks for; a transposed convolution x (Cin, d, h, w) -> (Cout, 2d, 2h, 2w) is the input gradient (which 1) of the stride-2
// convolution (Ci = Cout, Co = Cin, 2d, 2h, 2w).
extern "C" int mode_conv3d_split_shape_supported(int Ci, int Co, int D, int H, int W, int stride, int which) {
  if (D <= 0 || H <= 0 || W <= 0 || which < 0 || which > 2) return 0;
  if (mode_conv3d_split_supported(Ci, Co, stride, which) != 1) return 0;
  const long long DHW = (long long)D * H * W;
  if (stride == 1) {
    if (which == 2) return mode::conv3d_bww_split_fits(Ci, Co, DHW) ? 1 : 0;
    return mode::conv3d_s1_split_fits(which == 1 ? Ci : Co, DHW) ? 1 : 0;
  }
  if (which == 0) return mode::conv3d_s2_split_fits(DHW) ? 1 : 0;
  if (which == 2) return (D % 2 == 0 && H % 2 == 0 && W % 8 == 0 && mode::conv3d_bww_s2_split_fits(Ci, Co, D, H, W)) ? 1 : 0;
  return (D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && mode::deconv3d_split_fits(Ci, DHW / 8)) ? 1 : 0;  // (gy at half the volume -> gx)
}

extern "C" int mode_conv3d_fwd_split(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci,
                                     int D, int H, int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_split";
  int rc = check_split_args(x, w, y, wpack, B, Ci, D, H, W, Co, 1, 0, who);
  if (rc == MODE_OK && bn) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv3d_s1_split(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), who, bn);
}

// Training forward with the BatchNorm batch statistics of the output taken in the kernel's epilogue (no statistics pass over y):
// `stats` receives mode_conv3d_fwd_split_stats_partials() partial pairs per output channel followed by the Co pivots
// (>= mode_bn_workspace_bytes(Co) bytes: the BatchNorm workspace itself), to be handed to mode_bn_train_fwd_prestats.
extern "C" int mode_conv3d_fwd_split_stats_partials(void) { return mode::conv3d_split_stat_partials(); }

extern "C" int mode_conv3d_fwd_split_stats(const float* x, const float* w, float* y, float* wpack, float* stats, int B, int Ci, int D, int H,
                                           int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_split_stats";
  int rc = check_split_args(x, w, y, wpack, B, Ci, D, H, W, Co, 1, 0, who);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats, MODE_ERR_WORKSPACE, "%s: statistics workspace required", who);
  MODE_REQUIRE(B > 0, MODE_ERR_BAD_ARG, "%s: empty batch has no statistics", who);
  return mode::conv3d_s1_split(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), who, nullptr, stats);
}

// Stride-2 forward on the split-bf16 kernel of conv3d_split_s2.hip (also the input gradient of the transposed convolution, with
// w = its (Cin, Cout, 27) weight read as (Co = Cin, Ci = Cout)); needs mode_conv3d_split_supported(Ci, Co, 2, 0) == 1.
extern "C" int mode_conv3d_fwd_s2_split_amax(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* out_absmax, float* wpack,
                                             int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_s2_split";
  int rc = check_split_args(x, w, y, wpack, B, Ci, D, H, W, Co, 2, 0, who);
  if (rc == MODE_OK && bn) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(!out_absmax || bn, MODE_ERR_BAD_ARG, "%s: the output maximum comes out of the eval epilogue (bn is NULL)", who);
  if (B == 0) return out_absmax ? mode::absmax_begin(out_absmax, mode::as_stream(stream), who) : MODE_OK;
  return mode::conv3d_s2_split(x, w, y, wpack, B, Ci, Co, D, H, W, mode::as_stream(stream), who, bn, out_absmax);
}

extern "C" int mode_conv3d_fwd_s2_split(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci,
                                        int D, int H, int W, int Co, mode_stream_t stream) {
  return mode_conv3d_fwd_s2_split_amax(x, w, bn, y, nullptr, wpack, B, Ci, D, H, W, Co, stream);
}

// Input gradient of the stride-2 convolution = the transposed convolution of gy with the same (Co, Ci, 27) weight, on the split-bf16
// kernel of conv3d_split_deconv.hip; even D, H, W; needs mode_conv3d_split_supported(Ci, Co, 2, 1) == 1.
extern "C" int mode_conv3d_bwd_data_s2_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W,
                                             int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_data_s2_split";
  int rc = check_split_args(gy, w, gx, wpack, B, Ci, D, H, W, Co, 2, 1, who);  // (even D, H, W among the rest)
  if (rc != MODE_OK || B == 0) return rc;
  return mode::deconv3d_split(gy, w, gx, wpack, B, Co, Ci, D / 2, H / 2, W / 2, mode::as_stream(stream), who);
}

// ---- the stride-1 layer on the two-piece fp16 arithmetic (three MFMAs per product; csrc/conv3d_split.hip).  amax_*: device floats, the
// largest magnitude of each operand (mode_abs_max), read by the kernels themselves: no host synchronisation.
extern "C" int mode_abs_max(const float* x, long long n, float* out, mode_stream_t stream) {
  return mode::abs_max(x, n, out, mode::as_stream(stream), "mode_abs_max");
}

extern "C" int mode_abs_max_batch(const float* const* device_ptrs, const long long* device_sizes, int n, float* out, mode_stream_t stream) {
  return mode::abs_max_batch(device_ptrs, device_sizes, n, out, mode::as_stream(stream), "mode_abs_max_batch");
}

extern "C" int mode_conv3d_fwd_split_f16(const float* x, const float* w, const float* amax_x, const float* amax_w, float* y, float* wpack, int B,
                                         int Ci, int D, int H, int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_split_f16";
  int rc = check_split_args(x, w, y, wpack, B, Ci, D, H, W, Co, 1, 0, who);
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE(amax_x && amax_w, MODE_ERR_BAD_ARG, "%s: null operand maximum", who);
  return mode::conv3d_s1_split(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), who, nullptr, nullptr, nullptr, amax_x, amax_w);
}

// Eval mode on the fp16 arithmetic: y = relu?(bn(conv(x)) [+ add]) with the BatchNorm scale folded into the weights BEFORE they are scaled
// and split (their maximum is taken inside, where they are packed, and kept in wpack); amax_y receives the maximum of y for the next layer.
extern "C" int mode_conv3d_fwd_split_f16_bn(const float* x, const float* w, const float* amax_x, const mode_bn_epilogue* bn, float* y,
                                            float* amax_y, float* wpack, int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_split_f16_bn";
  int rc = check_split_args(x, w, y, wpack, B, Ci, D, H, W, Co, 1, 0, who);
  if (rc == MODE_OK) {
    MODE_REQUIRE(bn, MODE_ERR_BAD_ARG, "%s: null BatchNorm epilogue", who);
    rc = mode::check_bn(bn, who);
  }
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(amax_x && amax_y, MODE_ERR_BAD_ARG, "%s: null maximum buffer", who);
  if (B == 0) return mode::absmax_begin(amax_y, mode::as_stream(stream), who);  // (an empty output's maximum is zero)
  return mode::conv3d_s1_split(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), who, bn, nullptr, nullptr, amax_x, nullptr, amax_y);
}

// gx = conv^T(gy) [+ acc]; amax_g = max |gy|, amax_w = max |w|
extern "C" int mode_conv3d_bwd_data_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, const float* acc, float* gx,
                                              float* wpack, int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_data_split_f16";
  int rc = check_split_args(gy, w, gx, wpack, B, Ci, D, H, W, Co, 1, 1, who);
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE(amax_g && amax_w && acc != gx, MODE_ERR_BAD_ARG, "%s: null operand maximum, or acc is the output tensor", who);
  return mode::conv3d_s1_split(gy, w, gx, wpack, B, Co, Ci, D, H, W, 1, mode::as_stream(stream), who, nullptr, nullptr, acc, amax_g, amax_w);
}

// The two input gradients with a gradient that is already there added in the store: gx = conv^T(gy) + acc (acc must not alias gx).
extern "C" int mode_conv3d_bwd_data_split_acc_supported(int Ci, int Co, int stride) {
  if (Ci <= 0 || Co <= 0) return 0;
  if (stride == 1) return mode::conv3d_split_supported(Co, Ci) ? 1 : 0;
  return (stride == 2 && mode::deconv3d_split_bn_supported(Co, Ci)) ? 1 : 0;
}

extern "C" int mode_conv3d_bwd_data_split_acc(const float* gy, const float* w, const float* acc, float* gx, float* wpack, int B, int Ci, int D,
                                              int H, int W, int Co, int stride, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_data_split_acc";
  MODE_REQUIRE(stride == 1 || stride == 2, MODE_ERR_UNSUPPORTED, "%s: stride %d not implemented", who, stride);
  int rc = check_split_args(gy, w, gx, wpack, B, Ci, D, H, W, Co, stride, 1, who);  // (stride 2: even D, H, W among the rest)
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE(acc && acc != gx, MODE_ERR_BAD_ARG, "%s: acc must be a tensor of gx's shape that is not gx", who);
  if (stride == 1) return mode::conv3d_s1_split(gy, w, gx, wpack, B, Co, Ci, D, H, W, 1, mode::as_stream(stream), who, nullptr, nullptr, acc);
  return mode::deconv3d_split(gy, w, gx, wpack, B, Co, Ci, D / 2, H / 2, W / 2, mode::as_stream(stream), who, nullptr, acc);
}

// ConvTranspose3d k3 s2 p1 op1 on the same kernel: x (B, Cin, D, H, W), w (Cin, Cout, 27) -> y (B, Cout, 2D, 2H, 2W).
extern "C" int mode_deconv3d_split_supported(int Cin, int Cout) { return mode::deconv3d_split_supported(Cin, Cout) ? 1 : 0; }

extern "C" int mode_deconv3d_fwd_split(const float* x, const float* w, float* y, float* wpack, int B, int Cin, int D, int H, int W, int Cout,
                                       mode_stream_t stream) {
  const char* who = "mode_deconv3d_fwd_split";
  int rc = check_deconv_split_args(x, w, y, wpack, B, Cin, D, H, W, Cout, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::deconv3d_split(x, w, y, wpack, B, Cin, Cout, D, H, W, mode::as_stream(stream), who);
}

extern "C" int mode_deconv3d_split_bn_supported(int Cin, int Cout) { return mode::deconv3d_split_bn_supported(Cin, Cout) ? 1 : 0; }

extern "C" int mode_deconv3d_fwd_split_bn_amax(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* out_absmax,
                                               float* wpack, int B, int Cin, int D, int H, int W, int Cout, mode_stream_t stream) {
  const char* who = "mode_deconv3d_fwd_split_bn";
  int rc = check_deconv_split_args(x, w, y, wpack, B, Cin, D, H, W, Cout, who);
  if (rc == MODE_OK) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK) return rc;
  if (B == 0) return out_absmax ? mode::absmax_begin(out_absmax, mode::as_stream(stream), who) : MODE_OK;
  return mode::deconv3d_split(x, w, y, wpack, B, Cin, Cout, D, H, W, mode::as_stream(stream), who, bn, nullptr, out_absmax);
}

extern "C" int mode_deconv3d_fwd_split_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Cin,
                                          int D, int H, int W, int Cout, mode_stream_t stream) {
  return mode_deconv3d_fwd_split_bn_amax(x, w, bn, y, nullptr, wpack, B, Cin, D, H, W, Cout, stream);
}

extern "C" int mode_conv3d_bwd_data_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W,
                                          int Co, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_data_split";
  int rc = check_split_args(gy, w, gx, wpack, B, Ci, D, H, W, Co, 1, 1, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv3d_s1_split(gy, w, gx, wpack, B, Co, Ci, D, H, W, 1, mode::as_stream(stream), who, nullptr);
}

extern "C" int mode_conv3d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int D, int H, int W, int Co,
                               int stride, mode_stream_t stream) {
  int rc = check_conv_args(x, w, y, wpack, B, Ci, D, H, W, Co, stride, "mode_conv3d_fwd", true);
  if (rc != MODE_OK || B == 0) return rc;
  if (stride == 2) return mode::conv3d_s2(x, w, y, wpack, B, Ci, Co, D, H, W, mode::as_stream(stream), "mode_conv3d_fwd");
  if (Co == 1) return mode::conv3d_co1_fwd(x, w, y, B, Ci, D, H, W, mode::as_stream(stream), "mode_conv3d_fwd");
  return mode::conv3d_s1(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), "mode_conv3d_fwd");
}

extern "C" int mode_conv3d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci,
                                  int D, int H, int W, int Co, int stride, mode_stream_t stream) {
  const char* who = "mode_conv3d_fwd_bn";
  int rc = check_conv_args(x, w, y, wpack, B, Ci, D, H, W, Co, stride, who, true);
  if (rc == MODE_OK) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE(Co > 1, MODE_ERR_UNSUPPORTED, "%s: the single-output-channel kernels have no epilogue", who);
  if (stride == 2) return mode::conv3d_s2(x, w, y, wpack, B, Ci, Co, D, H, W, mode::as_stream(stream), who, bn);
  return mode::conv3d_s1(x, w, y, wpack, B, Ci, Co, D, H, W, 0, mode::as_stream(stream), who, bn);
}

extern "C" int mode_conv3d_bwd_data(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W,
                                    int Co, int stride, mode_stream_t stream) {
  int rc = check_conv_args(gy, w, gx, wpack, B, Ci, D, H, W, Co, stride, "mode_conv3d_bwd_data", true);
  if (rc != MODE_OK || B == 0) return rc;
  if (stride == 2) {
    // gx = transposed convolution of gy with the same weights, indexed w[o][c][tap] = w[cin_of_deconv][cout_of_deconv][tap]
    MODE_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, MODE_ERR_UNSUPPORTED,
                 "mode_conv3d_bwd_data: stride 2 needs even input sizes (got %dx%dx%d)", D, H, W);
    return mode::deconv3d(gy, w, gx, wpack, B, Co, Ci, D / 2, H / 2, W / 2, mode::as_stream(stream), "mode_conv3d_bwd_data");
  }
  if (Co == 1) return mode::conv3d_co1_bwd_data(gy, w, gx, B, Ci, D, H, W, mode::as_stream(stream), "mode_conv3d_bwd_data");
  return mode::conv3d_s1(gy, w, gx, wpack, B, Co, Ci, D, H, W, 1, mode::as_stream(stream), "mode_conv3d_bwd_data");
}

// ---- weight gradient: split-K partials in `workspace` (sized by the query below for the S of conv3d_wgrad_grid), then their reduction
extern "C" size_t mode_conv3d_bwd_weight_workspace_bytes(int B, int Ci, int D, int H, int W, int Co, int stride) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  const size_t generic = mode::conv3d_wgrad_grid(B, Ci, D, H, W, Co, stride).part_floats();
  const size_t co1 = (Co == 1 && stride == 1) ? mode::conv3d_co1_bwd_weight_workspace_floats(B, Ci, D, H, W) : 0;
  return std::max(generic, co1) * sizeof(float);
}

extern "C" int mode_conv3d_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H,
                                      int W, int Co, int stride, int accumulate, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_weight";
  int rc = check_conv_args(gy, x, gw, workspace, B, Ci, D, H, W, Co, stride, who, true);
  if (rc != MODE_OK) return rc;
  hipStream_t st = mode::as_stream(stream);
  if (B == 0) return empty_batch_gw(gw, Ci, Co, accumulate, st, who);
  if (Co == 1 && stride == 1) return mode::conv3d_co1_bwd_weight(gy, x, gw, workspace, B, Ci, D, H, W, accumulate, st, who);
  int S;
  rc = mode::conv3d_f32_wgrad_partials(gy, x, workspace, B, Ci, D, H, W, Co, stride, st, who, &S);
  if (rc != MODE_OK) return rc;
  return mode::conv3d_wgrad_reduce(workspace, gw, Ci, Co, S, accumulate, st, who);
}

namespace {

// The split-K partition of a rolling-window split kernel (q: its WgradSplitDims / WgradS2SplitDims) over `columns` columns of `depth`
// depths: the depths per work unit (ring_depths), the units, and the slices -- S wanted, at most one per unit and never more than
// `sized`, the slices the workspace query assumed.
template <typename Q>
void ring_partition(Q& q, int depth, long long columns, int floor, int S, int sized) {
  q.ring_dc = mode::ring_depths(depth, columns, S, floor);
  q.nDc = mode::cdiv(depth, q.ring_dc);
  q.units = (int)(columns * q.nDc);
  q.S = std::min(std::min(S, q.units), sized);
}

int bwd_weight_split(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw, float* workspace, int B, int Ci,
                     int D, int H, int W, int Co, int accumulate, mode_stream_t stream, const char* who) {
  int rc = check_split_args(gy, x, gw, workspace, B, Ci, D, H, W, Co, 1, 2, who);
  if (rc != MODE_OK) return rc;
  hipStream_t st = mode::as_stream(stream);
  if (B == 0) return empty_batch_gw(gw, Ci, Co, accumulate, st, who);
  const mode::WgradGrid g = mode::conv3d_wgrad_grid(B, Ci, D, H, W, Co, 1);
  mode::WgradSplitDims q;
  q.Ci = Ci; q.Co = Co; q.D = D; q.H = H; q.W = W;
  q.nWt = g.nWt; q.nHt = g.nHt; q.MTo = g.MTo; q.MTc = g.MTc;
  // one workgroup per CU and (o, c) block pair (152 KB of LDS each); depths per unit as for the fp32 ring kernel
  ring_partition(q, D, (long long)B * g.nHt * g.nWt, 6, mode::cdiv(kNumCU, g.MTo * g.MTc), g.S);
  rc = mode::conv3d_bww_split_launch(gy, x, workspace, q, st, who, amax_g, amax_x);
  if (rc != MODE_OK) return rc;
  return mode::conv3d_wgrad_reduce(workspace, gw, Ci, Co, q.S, accumulate, st, who);
}

}  // namespace

extern "C" int mode_conv3d_bwd_weight_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H,
                                            int W, int Co, int accumulate, mode_stream_t stream) {
  return bwd_weight_split(gy, x, nullptr, nullptr, gw, workspace, B, Ci, D, H, W, Co, accumulate, stream, "mode_conv3d_bwd_weight_split");
}

// The same on the two-piece fp16 arithmetic (mode_conv3d_fwd_split_f16): amax_g / amax_x = device floats max |gy| / max |x|
extern "C" int mode_conv3d_bwd_weight_split_f16(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw, float* workspace,
                                                int B, int Ci, int D, int H, int W, int Co, int accumulate, mode_stream_t stream) {
  MODE_REQUIRE(amax_g && amax_x, MODE_ERR_BAD_ARG, "mode_conv3d_bwd_weight_split_f16: null operand maximum");
  return bwd_weight_split(gy, x, amax_g, amax_x, gw, workspace, B, Ci, D, H, W, Co, accumulate, stream, "mode_conv3d_bwd_weight_split_f16");
}

// Weight gradient of the stride-2 convolution on the split-bf16 kernel of conv3d_split_wgrad_s2.hip: x (B, Ci, D, H, W), gy (B, Co,
// D/2, H/2, W/2); D and H even, W a multiple of 8; needs mode_conv3d_split_supported(Ci, Co, 2, 2) == 1.  With (gy := the input of a
// ConvTranspose3d, x := the gradient of its output) the result is that layer's (Cin, Cout, 27) weight gradient.
extern "C" int mode_conv3d_bwd_weight_s2_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H,
                                               int W, int Co, int accumulate, mode_stream_t stream) {
  const char* who = "mode_conv3d_bwd_weight_s2_split";
  int rc = check_split_args(gy, x, gw, workspace, B, Ci, D, H, W, Co, 2, 2, who);  // (even D, H and W a multiple of 8 among the rest)
  if (rc != MODE_OK) return rc;
  hipStream_t st = mode::as_stream(stream);
  if (B == 0) return empty_batch_gw(gw, Ci, Co, accumulate, st, who);
  const mode::WgradGrid g = mode::conv3d_wgrad_grid(B, Ci, D, H, W, Co, 2);
  mode::WgradS2SplitDims q;
  q.Ci = Ci; q.Co = Co; q.D = D; q.H = H; q.W = W; q.Do = g.Do; q.Ho = g.Ho; q.Wo = g.Wo;
  q.nWt = mode::cdiv(g.Wo, 16); q.MTo = g.MTo; q.MTc = g.MTc;
  // one workgroup per CU (130 KB of LDS each); a unit starts with two un-pipelined stagings, so as deep as the volume allows while
  // every workgroup still gets >= 2 units
  ring_partition(q, g.Do, (long long)B * g.Ho * q.nWt, 3, std::max(1, kNumCU / (mode::cdiv(g.MTo, 2) * g.MTc)), g.S);
  rc = mode::conv3d_bww_s2_split_launch(gy, x, workspace, q, st, who);
  if (rc != MODE_OK) return rc;
  return mode::conv3d_wgrad_reduce(workspace, gw, Ci, Co, q.S, accumulate, st, who);
}

// Transposed convolution k3 s2 p1 op1 (= backward-data of the stride-2 convolution) on the fp32 kernel:
//   x (B, Cin, D, H, W), w the ConvTranspose3d weight (Cin, Cout, 3,3,3) -> y (B, Cout, 2D, 2H, 2W)
extern "C" int mode_deconv3d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Cin, int D, int H, int W,
                                 int Cout, mode_stream_t stream) {
  int rc = check_conv_args(x, w, y, wpack, B, Cin, D, H, W, Cout, 1, "mode_deconv3d_fwd");
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE((long long)Cout * D * H * W * 8 < (1ll << 31), MODE_ERR_UNSUPPORTED, "mode_deconv3d_fwd: output sample too large");
  return mode::deconv3d(x, w, y, wpack, B, Cin, Cout, D, H, W, mode::as_stream(stream), "mode_deconv3d_fwd");
}

extern "C" int mode_deconv3d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Cin,
                                    int D, int H, int W, int Cout, mode_stream_t stream) {
  const char* who = "mode_deconv3d_fwd_bn";
  int rc = check_conv_args(x, w, y, wpack, B, Cin, D, H, W, Cout, 1, who);
  if (rc == MODE_OK) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK || B == 0) return rc;
  MODE_REQUIRE((long long)Cout * D * H * W * 8 < (1ll << 31), MODE_ERR_UNSUPPORTED, "%s: output sample too large", who);
  return mode::deconv3d(x, w, y, wpack, B, Cin, Cout, D, H, W, mode::as_stream(stream), who, bn);
}
