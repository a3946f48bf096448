// The 32-bit size contracts of the split-operand convolution kernels, in ONE place (host arithmetic only).  Every launching
// entry of these kernels, the two ABI predicates mode_conv3d_split_shape_supported / mode_conv2d_split_shape_supported and -- through
// them -- the Python dispatchers ask the functions below; nothing else spells these inequalities.
//
// Common ground (common.h: buf_rsrc / kBufOOB).  The kernels stage their operands with raw buffer loads: a descriptor of `bytes`
// bytes, a 32-bit lane offset, and a lane offset at or beyond `bytes` reads as zero.  A position in the zero padding is given a
// SENTINEL offset instead of its own.  That is right exactly while
//     largest valid lane offset  <  descriptor bytes  <  smallest sentinel  <  2^32,
// all four as the 32-bit values the kernel computes -- `bytes` is an `unsigned` product in the kernels and wraps silently.  The middle
// inequality is kept strict, as common.h states the contract (bytes < 2^31): a descriptor that ends exactly on the sentinel would lean
// on the hardware's range check comparing with >= and on the scalar offset taking no part in it.
#pragma once
#include <algorithm>

namespace mode {

constexpr long long kLaneSentinel = 1ll << 31;  // kBufOOB
constexpr long long kHalfSentinel = 1ll << 30;  // kHalfOOB of conv2d_split_wgrad.hip

// Stride-1 3-D split, forward / input gradient / eval epilogues, both arithmetics (conv3d_split.hip, stage_begin / stage_load):
//   descriptor = the chunk's 8 channel planes = 32 * DHW bytes (K is a multiple of 8, so a chunk is always 8 whole planes);
//   valid lane offset = 4 * voxel < 4 * DHW;  sentinel = kBufOOB = 2^31.
// -> 32 * DHW < 2^31.  The epilogue indexes a sample of the output with rows * DHW < 2^31 elements (as before).
inline bool conv3d_s1_split_fits(int rows, long long DHW) { return 32 * DHW < kLaneSentinel && rows * DHW < (1ll << 31); }

// Stride-2 3-D split forward (conv3d_split_s2.hip): the same descriptor over the INPUT volume D x H x W.
inline bool conv3d_s2_split_fits(long long DHW) { return 32 * DHW < kLaneSentinel; }

// Transposed split (conv3d_split_deconv.hip): the same descriptor over its LOW-resolution input of DHW voxels.  The second condition
// is the entry's sample limit from before the buffer loads -- an output sample of 8 * DHW voxels in max(Co, 8) channels below 2^31
// elements, what the fp32 kernel behind the fallback takes as well; the epilogue's own offsets are 64-bit.  It implies the first.
inline bool deconv3d_split_fits(int Co, long long DHW) { return 32 * DHW < kLaneSentinel && 8 * DHW * std::max(Co, 8) < (1ll << 31); }

// Stride-1 3-D split weight gradient (conv3d_split_wgrad.hip, unit_begin / load_x / load_g):
//   descriptor = block_bytes = 128 * DHW: 32 channel planes of a sample, WHATEVER the layer's channel count (channels beyond it are
//   masked by the sentinel, not by the descriptor) -- a 16 -> 16 layer wraps `block_bytes` at the same volume as a 32 -> 32 one;
//   valid lane offset = 4 * (c * DHW + row * W + col) (+ 4) <= 4 * (31 * DHW + HW), the plane is the scalar offset;  sentinel = 2^31.
// -> 128 * DHW < 2^31.  The work split and the reduction keep max(Ci, Co) * DHW < 2^29 (32-bit element offsets, as before).
inline bool conv3d_bww_split_fits(int Ci, int Co, long long DHW) {
  return 128 * DHW < kLaneSentinel && std::max(Ci, Co) * DHW < (1ll << 29);
}

// Stride-2 3-D split weight gradient (conv3d_split_wgrad_s2.hip): no buffer loads; unsigned BYTE offsets inside a 32-channel block of x
// (D x H x W) and a 64-channel block of gy (half of it each way) -- 4 * 32 * DHW and 4 * 64 * oDHW below 2^31.
inline bool conv3d_bww_s2_split_fits(int Ci, int Co, int D, int H, int W) {
  return std::max((long long)std::min(Ci, 32) * D * H * W, (long long)std::min(Co, 64) * (D / 2) * (H / 2) * (W / 2)) < (1ll << 29);
}

// 2-D split forward / input gradient (conv2d_split.hip): descriptor = the chunk's 16 channel planes = 64 * HW bytes (K is a multiple of
// 16), valid lane offset < 4 * HW, sentinel 2^31 -> 64 * HW < 2^31; the epilogue keeps max(K, rows) * HW < 2^29 (as before; with
// K >= 16 it implies the first).
inline bool conv2d_split_fits(int K, int rows, long long HW) { return 64 * HW < kLaneSentinel && std::max(K, rows) * HW < (1ll << 29); }

// 2-D split weight gradient (conv2d_split_wgrad.hip, unit_begin / load_x / load_g).  The lane offset is a SUM of a column part and a
// row part, each either a valid byte offset or the marker kHalfOOB = 2^30:
//   descriptor = block_bytes = 128 * HW (32 channel planes, whatever the channel count);
//   column part: 4 * (c * HW + row_in_group * W + col) (+ 4), valid;  row part: 4 * r0 * W with r0 the first row of the staged group of
//   four -- r0 >= -dilation, NEGATIVE for the top halo; a valid pair sums to 4 * (c * HW + row * W + col) < 128 * HW;
//   invalid column, valid row:  2^30 + 4 * r0 * W  >=  2^30 - 4 * dilation * W      <- the smallest sentinel
//   valid column, invalid row:  2^30 + column part  <  2^30 + 128 * HW;   both invalid: 2^31.
// -> 128 * HW < 2^30 - 4 * dilation * W (and then every sum stays below 2^32).  max(Ci, Co) * HW < 2^29 as before.
inline bool conv2d_bww_split_fits(int Ci, int Co, int H, int W, int dilation) {
  const long long HW = (long long)H * W;
  return 128 * HW < kHalfSentinel - 4ll * dilation * W && std::max(Ci, Co) * HW < (1ll << 29);
}

}  // namespace mode
