// The C entries of the regular 3x3 Conv2d family (stride 1, padding = dilation in {1, 2}, no bias: nn.Conv2d inside convbn,
// models/submodule.py:15-17 -- 31 of the extractor's 39 Conv2d layers, and the fusion network) and their argument checks.
// Pure host code; the kernels, each with the host function that launches it (conv2d_internal.h), are in
//   conv2d_f32_fwd.hip          fp32 MFMA: pack_w2d, conv2d_kernel (forward, and the input gradient on flipped weights); zero_insert2_kernel
//   conv2d_f32_wgrad.hip        fp32 MFMA: conv2d_bwd_weight_kernel; reduce_gw2d (every weight gradient's partials)
//   conv2d_split.hip            split operands (bf16 x 3, fp16 x 2): forward / input gradient, eval epilogues
//   conv2d_split_wgrad.hip      ... weight gradient
#include "common.h"
#include "bn_internal.h"
#include "conv2d_internal.h"

namespace {

enum Family { F32, SPLIT };  // which kernels an entry launches: the fp32 MFMA ones, or the split-operand ones

// One check for every entry, in ONE order: sizes (MODE_ERR_BAD_ARG); dilation in {1, 2}; the size rule of the kernel that the entry
// launches for `which` (0 forward, 1 input gradient, 2 weight gradient; both MODE_ERR_UNSUPPORTED); pointers last (MODE_ERR_BAD_ARG),
// and none needed for an empty batch: a shape beyond a limit is unsupported whatever the pointers are.  What concerns one entry alone
// (a maximum, an epilogue, acc) follows in that entry.
int check_args(const void* a, const void* b, const void* c, const void* wp, int B, int Ci, int H, int W, int Co, int dilation, Family family,
               int which, const char* who) {
  MODE_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: non-positive size", who);
  MODE_REQUIRE(dilation == 1 || dilation == 2, MODE_ERR_UNSUPPORTED, "%s: dilation %d not implemented (1 or 2)", who, dilation);
  if (family == SPLIT) {
    MODE_REQUIRE(mode_conv2d_split_shape_supported(Ci, Co, H, W, dilation, which) == 1, MODE_ERR_UNSUPPORTED, "%s: %d -> %d channels at %dx%d: "
                 "not covered by the split kernel, or beyond its 32-bit offsets (mode_conv2d_split_shape_supported)", who, Ci, Co, H, W);
  } else {
    const int rows = which == 0 ? Co : which == 1 ? Ci : 0;  // output channels of a forward / input gradient; the weight gradient takes any
    MODE_REQUIRE(rows <= 128, MODE_ERR_UNSUPPORTED, "%s: more than 128 output channels (%d) not supported", who, rows);
    MODE_REQUIRE((long long)std::max(Ci, Co) * H * W < (1ll << 29), MODE_ERR_UNSUPPORTED, "%s: a sample larger than 2^29 elements", who);
  }
  if (B == 0) return MODE_OK;
  MODE_REQUIRE(a && b && c && wp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  return MODE_OK;
}

// The weight gradient of an empty batch is zero: written unless the call accumulates.
int empty_batch_gw(float* gw, int Ci, int Co, int accumulate, hipStream_t st, const char* who) {
  return accumulate ? MODE_OK : mode::zero_floats(gw, (size_t)Co * Ci * 9, st, who);
}

}  // namespace

extern "C" size_t mode_conv2d_wpack_bytes(int Ci, int Co) {
  if (Ci <= 0 || Co <= 0) return 0;
  const size_t f = mode::conv2d_f32_pack_floats(Ci, Co), b = mode::conv2d_f32_pack_floats(Co, Ci);  // forward, input gradient
  size_t n = (f > b ? f : b) + 32 * (size_t)mode::cdiv(Co > Ci ? Co : Ci, 32);  // + the folded BatchNorm shifts
  n = std::max(n, std::max(mode::conv2d_split_wpack_floats(Ci, Co), mode::conv2d_split_wpack_floats(Co, Ci)));
  return n * sizeof(float);
}

extern "C" int mode_conv2d_split_supported(int Ci, int Co, int dilation, int which) {
  if (Ci <= 0 || Co <= 0) return 0;
  return which == 1 ? mode::conv2d_split_supported(Co, Ci, dilation) : mode::conv2d_split_supported(Ci, Co, dilation);
}

// Host only, launches nothing: 1 exactly when the layer is supported (which 0 / 1: mode_conv2d_split_supported; the weight gradient,
// which 2, takes any channel counts in masked 32 x 32 blocks) AND the image is inside every 32-bit contract of the kernel that the
// corresponding split entry launches (size_contracts.h has the derivations).
extern "C" int mode_conv2d_split_shape_supported(int Ci, int Co, int H, int W, int dilation, int which) {
  if (Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || (dilation != 1 && dilation != 2)) return 0;
  if (which == 2) return mode::conv2d_bww_split_fits(Ci, Co, H, W, dilation) ? 1 : 0;
  if (which != 0 && which != 1) return 0;
  if (mode_conv2d_split_supported(Ci, Co, dilation, which) != 1) return 0;
  return mode::conv2d_split_fits(which == 1 ? Co : Ci, which == 1 ? Ci : Co, (long long)H * W) ? 1 : 0;
}

// ---- forward and input gradient on the split kernels (conv2d_split.hip); bn: the optional folded-BatchNorm epilogue of an eval layer
extern "C" int mode_conv2d_fwd_split(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H,
                                     int W, int Co, int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_fwd_split";
  int rc = check_args(x, w, y, wpack, B, Ci, H, W, Co, dilation, SPLIT, 0, who);
  if (rc == MODE_OK && bn) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv2d_split_run(x, w, y, wpack, B, Ci, Co, H, W, dilation, 0, mode::as_stream(stream), who, bn);
}

extern "C" int mode_conv2d_bwd_data_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int H, int W, int Co,
                                          int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_bwd_data_split";
  int rc = check_args(gy, w, gx, wpack, B, Ci, H, W, Co, dilation, SPLIT, 1, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv2d_split_run(gy, w, gx, wpack, B, Co, Ci, H, W, dilation, 1, mode::as_stream(stream), who, nullptr);
}

// gx = conv^T(gy) + acc: a gradient of the same tensor that is already there, added in the store (acc must not alias gx)
extern "C" int mode_conv2d_bwd_data_split_acc(const float* gy, const float* w, const float* acc, float* gx, float* wpack, int B, int Ci, int H,
                                              int W, int Co, int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_bwd_data_split_acc";
  int rc = check_args(gy, w, gx, wpack, B, Ci, H, W, Co, dilation, SPLIT, 1, who);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(acc && acc != gx, MODE_ERR_BAD_ARG, "%s: acc must be a tensor of gx's shape that is not gx", who);
  if (B == 0) return MODE_OK;
  return mode::conv2d_split_run(gy, w, gx, wpack, B, Co, Ci, H, W, dilation, 1, mode::as_stream(stream), who, nullptr, acc);
}

// The two calls of a TRAINING step on the two-piece fp16 arithmetic (conv3d_split.hip): amax_* = the maximum buffers
// (MODE_BN_ABSMAX_FLOATS floats) of the activation / gradient and of the weight; acc may be NULL.
extern "C" int mode_conv2d_fwd_split_f16(const float* x, const float* w, const float* amax_x, const float* amax_w, float* y, float* wpack, int B,
                                         int Ci, int H, int W, int Co, int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_fwd_split_f16";
  int rc = check_args(x, w, y, wpack, B, Ci, H, W, Co, dilation, SPLIT, 0, who);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(amax_x && amax_w, MODE_ERR_BAD_ARG, "%s: null maximum", who);
  if (B == 0) return MODE_OK;
  return mode::conv2d_split_run(x, w, y, wpack, B, Ci, Co, H, W, dilation, 0, mode::as_stream(stream), who, nullptr, nullptr, amax_x, amax_w);
}

extern "C" int mode_conv2d_bwd_data_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, const float* acc,
                                              float* gx, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                                              mode_stream_t stream) {
  const char* who = "mode_conv2d_bwd_data_split_f16";
  int rc = check_args(gy, w, gx, wpack, B, Ci, H, W, Co, dilation, SPLIT, 1, who);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(amax_g && amax_w && !(acc && acc == gx), MODE_ERR_BAD_ARG, "%s: null maximum, or acc is the output tensor", who);
  if (B == 0) return MODE_OK;
  return mode::conv2d_split_run(gy, w, gx, wpack, B, Co, Ci, H, W, dilation, 1, mode::as_stream(stream), who, nullptr, acc, amax_g, amax_w);
}

// Inference on the same arithmetic (ABI 31; mode_conv3d_fwd_split_f16_bn is the 3-D twin): folded BatchNorm (+ residual) (+ ReLU), the
// folded weights' maximum taken inside with the pack, the stored output's maximum left in amax_y for the next layer.
extern "C" int mode_conv2d_fwd_split_f16_bn(const float* x, const float* w, const float* amax_x, const mode_bn_epilogue* bn, float* y,
                                            float* amax_y, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                                            mode_stream_t stream) {
  const char* who = "mode_conv2d_fwd_split_f16_bn";
  int rc = check_args(x, w, y, wpack, B, Ci, H, W, Co, dilation, SPLIT, 0, who);
  if (rc == MODE_OK) {
    MODE_REQUIRE(bn, MODE_ERR_BAD_ARG, "%s: null BatchNorm epilogue", who);
    rc = mode::check_bn(bn, who);
  }
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(amax_x && amax_y, MODE_ERR_BAD_ARG, "%s: null maximum buffer", who);
  if (B == 0) return mode::absmax_begin(amax_y, mode::as_stream(stream), who);  // (an empty output's maximum is zero)
  return mode::conv2d_split_run(x, w, y, wpack, B, Ci, Co, H, W, dilation, 0, mode::as_stream(stream), who, bn, nullptr, amax_x, nullptr, amax_y);
}

// ---- forward and input gradient on the fp32 kernel (conv2d_f32_fwd.hip)
extern "C" int mode_conv2d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                               mode_stream_t stream) {
  const char* who = "mode_conv2d_fwd";
  int rc = check_args(x, w, y, wpack, B, Ci, H, W, Co, dilation, F32, 0, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv2d_f32_run(x, w, y, wpack, B, Ci, Co, H, W, dilation, 0, mode::as_stream(stream), who);
}

extern "C" int mode_conv2d_bwd_data(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int H, int W, int Co,
                                    int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_bwd_data";
  int rc = check_args(gy, w, gx, wpack, B, Ci, H, W, Co, dilation, F32, 1, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv2d_f32_run(gy, w, gx, wpack, B, Co, Ci, H, W, dilation, 1, mode::as_stream(stream), who);
}

extern "C" int mode_conv2d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H,
                                  int W, int Co, int dilation, mode_stream_t stream) {
  const char* who = "mode_conv2d_fwd_bn";
  int rc = check_args(x, w, y, wpack, B, Ci, H, W, Co, dilation, F32, 0, who);
  if (rc == MODE_OK) rc = mode::check_bn(bn, who);
  if (rc != MODE_OK || B == 0) return rc;
  return mode::conv2d_f32_run(x, w, y, wpack, B, Ci, Co, H, W, dilation, 0, mode::as_stream(stream), who, bn);
}

// ---- weight gradient: split-K partials in `workspace` (sized by the query below for the S of conv2d_wgrad_grid), then their reduction
extern "C" size_t mode_conv2d_bwd_weight_workspace_bytes(int B, int Ci, int H, int W, int Co) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return 0;
  return mode::conv2d_wgrad_grid(B, Ci, H, W, Co).part_floats() * sizeof(float);
}

extern "C" int mode_conv2d_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                                      int dilation, int accumulate, mode_stream_t stream) {
  const char* who = "mode_conv2d_bwd_weight";
  int rc = check_args(gy, x, gw, workspace, B, Ci, H, W, Co, dilation, F32, 2, who);
  if (rc != MODE_OK) return rc;
  hipStream_t st = mode::as_stream(stream);
  if (B == 0) return empty_batch_gw(gw, Ci, Co, accumulate, st, who);
  int S;
  rc = mode::conv2d_f32_wgrad_partials(gy, x, workspace, B, Ci, H, W, Co, dilation, st, who, &S);
  if (rc != MODE_OK) return rc;
  return mode::conv2d_wgrad_reduce(workspace, gw, Ci, Co, S, accumulate, st, who);
}

namespace {

// The split-K partition of the split kernel (ring_partition of conv3d.hip, one dimension down) over B * nWt column strips of nGroups
// 4-row groups: a unit starts with an un-pipelined prologue, so runs as long as the image allows (halved while above 4 groups) while
// every one of the S workgroups wanted still gets a unit; S at most one per unit and never more than `sized`, the slices the
// workspace query assumed.
void run_partition(mode::Wgrad2SplitDims& q, int B, int S, int sized) {
  int run = q.nGroups;
  while (run > 4 && (long long)B * q.nWt * mode::cdiv(q.nGroups, run) < S) run = mode::cdiv(run, 2);
  q.run_groups = run;
  q.nRun = mode::cdiv(q.nGroups, run);
  q.units = B * q.nWt * q.nRun;
  q.S = std::min(std::min(S, q.units), sized);
}

int bwd_weight_split(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw, float* workspace, int B, int Ci,
                     int H, int W, int Co, int dilation, int accumulate, mode_stream_t stream, const char* who) {
  int rc = check_args(gy, x, gw, workspace, B, Ci, H, W, Co, dilation, SPLIT, 2, who);
  if (rc != MODE_OK) return rc;
  hipStream_t st = mode::as_stream(stream);
  if (B == 0) return empty_batch_gw(gw, Ci, Co, accumulate, st, who);
  const mode::Wgrad2Grid g = mode::conv2d_wgrad_grid(B, Ci, H, W, Co);
  mode::Wgrad2SplitDims q;
  q.Ci = Ci; q.Co = Co; q.H = H; q.W = W;
  q.nWt = g.nWt; q.MTo = g.MTo; q.MTc = g.MTc;
  q.nGroups = mode::cdiv(H, 4);
  run_partition(q, B, mode::cdiv(kNumCU, g.MTo * g.MTc), g.S);  // (one workgroup per CU and (o, c) block pair)
  rc = mode::conv2d_bww_split_launch(gy, x, workspace, q, dilation, st, who, amax_g, amax_x);
  if (rc != MODE_OK) return rc;
  return mode::conv2d_wgrad_reduce(workspace, gw, Ci, Co, q.S, accumulate, st, who);
}

}  // namespace

extern "C" int mode_conv2d_bwd_weight_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                                            int dilation, int accumulate, mode_stream_t stream) {
  return bwd_weight_split(gy, x, nullptr, nullptr, gw, workspace, B, Ci, H, W, Co, dilation, accumulate, stream, "mode_conv2d_bwd_weight_split");
}

// The same on the two-piece fp16 arithmetic (mode_conv2d_fwd_split_f16): amax_g / amax_x = the maximum buffers of gy and of x.
extern "C" int mode_conv2d_bwd_weight_split_f16(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw,
                                                float* workspace, int B, int Ci, int H, int W, int Co, int dilation, int accumulate,
                                                mode_stream_t stream) {
  MODE_REQUIRE(amax_g && amax_x, MODE_ERR_BAD_ARG, "mode_conv2d_bwd_weight_split_f16: null maximum");
  return bwd_weight_split(gy, x, amax_g, amax_x, gw, workspace, B, Ci, H, W, Co, dilation, accumulate, stream, "mode_conv2d_bwd_weight_split_f16");
}

// ---- zero insertion (conv2d_f32_fwd.hip): the two gradients of the extractor's one stride-2 3x3 layer are stride-1 gradients of its result
extern "C" int mode_zero_insert2(const float* in, float* out, long long planes, int Ho, int Wo, mode_stream_t stream) {
  MODE_REQUIRE(planes >= 0 && Ho > 0 && Wo > 0, MODE_ERR_BAD_ARG, "mode_zero_insert2: non-positive size");
  MODE_REQUIRE(Wo % 2 == 0, MODE_ERR_UNSUPPORTED, "mode_zero_insert2: the input width must be even (got %d)", Wo);
  if (planes == 0) return MODE_OK;
  MODE_REQUIRE(in && out, MODE_ERR_BAD_ARG, "mode_zero_insert2: null pointer");
  MODE_REQUIRE(((size_t)in % 8) == 0 && ((size_t)out % 16) == 0, MODE_ERR_UNSUPPORTED, "mode_zero_insert2: unaligned tensors");
  return mode::zero_insert2(in, out, planes, Ho, Wo, mode::as_stream(stream), "mode_zero_insert2");
}
