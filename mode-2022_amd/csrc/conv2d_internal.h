// Internal (non-ABI) entry points shared between the conv2d translation units (the regular 3x3 Conv2d family; conv2d.hip lists the files).
#pragma once
#include "common.h"
#include "size_contracts.h"

namespace mode {

#pragma GCC visibility push(hidden)  // (what moved out of an anonymous namespace stays out of the library's dynamic symbols)
// conv2d_f32_fwd.hip: the 3x3 layers on the fp32 MFMA.  rows = output channels of THIS GEMM (Co forward, Ci for the input gradient),
// K = its reduction channels; flip: how `w` is indexed (pack_w2d: 0 forward, 1 input gradient); bn: the folded-BatchNorm epilogue of an
// eval-mode layer.  wpack >= conv2d_f32_pack_floats(K, rows) + 32 * cdiv(rows, 32) floats.  Arguments are checked by the entry (conv2d.hip).
size_t conv2d_f32_pack_floats(int K, int rows);
int conv2d_f32_run(const float* x, const float* w, float* y, float* wpack, int B, int K, int rows, int H, int W, int dilation, int flip,
                   hipStream_t st, const char* who, const mode_bn_epilogue* bn = nullptr);
// out (planes, 2 Ho, 2 Wo) = in (planes, Ho, Wo) with zeros between (even Wo, in 8-byte and out 16-byte aligned)
int zero_insert2(const float* in, float* out, long long planes, int Ho, int Wo, hipStream_t st, const char* who);

// conv2d_f32_wgrad.hip: the weight gradient as split-K partials part[s][o / 32][c / 32][tap][o % 32][c % 32] and their reduction.
// The grid: tiles of 4 rows x 32 pixels, 32 x 32 channel blocks, and S = the split-K slices the workspace is sized for -- a launcher
// may write fewer slices, never more.  conv2d_f32_wgrad_partials: the fp32 kernel writes its partials, *S = the slices it wrote;
// conv2d_wgrad_reduce: gw[o][c][tap] (+)= the sum of the S slices, in a fixed order.
struct Wgrad2Grid {
  int nHt, nWt, MTo, MTc, S;
  size_t part_floats() const { return (size_t)S * MTo * MTc * 9 * 1024; }
};
Wgrad2Grid conv2d_wgrad_grid(int B, int Ci, int H, int W, int Co);
int conv2d_f32_wgrad_partials(const float* gy, const float* x, float* part, int B, int Ci, int H, int W, int Co, int dilation,
                              hipStream_t st, const char* who, int* S);
int conv2d_wgrad_reduce(const float* part, float* gw, int Ci, int Co, int S, int accumulate, hipStream_t st, const char* who);
#pragma GCC visibility pop

// conv2d_split.hip: the same layers on the split-bf16 matrix path; arguments as conv2d_f32_run.  The entry has checked sizes and
// pointers; what this checks is which optional arguments come together: acc_in (y = conv(x) + acc_in) not with bn; amax_x / amax_w (both
// or neither): the two-piece fp16 arithmetic; with bn (eval): amax_x and amax_y (the stored output's maximum, out), no amax_w -- the
// folded weights' maximum is taken with the pack and kept in wpack.
bool conv2d_split_supported(int K, int rows, int dilation);
size_t conv2d_split_wpack_floats(int K, int rows);
int conv2d_split_run(const float* x, const float* w, float* y, float* wpack, int B, int K, int rows, int H, int W, int dilation, int flip,
                     hipStream_t st, const char* who, const mode_bn_epilogue* bn, const float* acc_in = nullptr,
                     const float* amax_x = nullptr, const float* amax_w = nullptr, float* amax_y = nullptr);

// conv2d_split_wgrad.hip: split-K partials of the weight gradient on the split-bf16 path, in the layout of conv2d_f32_wgrad.hip; the
// caller reduces them (conv2d_wgrad_reduce).
struct Wgrad2SplitDims {
  int Ci, Co, H, W;
  int nWt, nGroups, run_groups, nRun, units;  // units = B * nWt * nRun runs of run_groups 4-row groups x 32 columns
  int S, MTo, MTc;
};
int conv2d_bww_split_launch(const float* gy, const float* x, float* part, const Wgrad2SplitDims& d, int dilation, hipStream_t st,
                            const char* who, const float* amax_g = nullptr, const float* amax_x = nullptr);

}  // namespace mode
