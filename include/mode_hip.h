/*
 * mode_hip.h -- C-ABI of libmode_hip.so: the MI355X (gfx950) kernels of MODE's disparity-stage hot path.
 *
 * Drop-in boundary.  The reference binds its native code through a two-function pybind11 module
 * (models/basic/spherical_conv/src/sphere_conv_cuda.cpp:339-345) that takes ATen tensors.  This
 * library is what a reference-side binding (ctypes / pybind / cgo) binds instead: plain device
 * pointers, sizes and a HIP stream -- no torch types.  Each entry point cites the reference
 * interface it replaces; paths are relative to the upstream repository root.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to a contiguous fp32 buffer allocated by the caller
 *     (the reference requires contiguous tensors too: sphere_conv_cuda.cpp:48, 138-140), unless
 *     the entry says otherwise (index and table buffers; the 8-bit frames of the ingest entries);
 *   - the library never allocates or keeps device memory; scratch is passed in as `workspace`;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *     the call returns without synchronising (reference: at::cuda::getCurrentCUDAStream(),
 *     sphere_conv_cuda_kernel.cu:280, 374);
 *   - the return value is MODE_OK (0) or a negative MODE_ERR_* code for rejected arguments /
 *     a positive hipError_t for a launch failure; mode_last_error() returns a description.  The
 *     reference throws c10::Error on bad shapes (sphere_conv_cuda.cpp:43-125) but only printf()s
 *     launch errors (sphere_conv_cuda_kernel.cu:286-289); the Python binding raises RuntimeError
 *     for every non-zero code;
 *   - re-entrant across devices and threads: no global mutable state except two thread-local
 *     values, the error string and the mode_weight_pack_reuse setting (nn.DataParallel calls
 *     forward from one thread per GPU).
 */
#ifndef MODE_HIP_H_
#define MODE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mode_stream_t; /* hipStream_t */

enum {
  MODE_OK = 0,
  MODE_ERR_BAD_ARG = -1,      /* NULL pointer, non-positive size, inconsistent shapes */
  MODE_ERR_UNSUPPORTED = -2,  /* valid request outside what the kernels implement */
  MODE_ERR_WORKSPACE = -3     /* workspace missing or too small */
};

/* Eval-mode epilogue of the *_bn entry points: the BatchNorm that follows a convolution in every convbn / convbn_3d /
 * sphereConvbn block (models/submodule.py:15-22, 61-74), in inference mode (running statistics), folded into the convolution:
 *     out = relu?( conv(x, w)[o] * gamma[o] / sqrt(var[o] + eps) + beta[o] - mean[o] * gamma[o] / sqrt(var[o] + eps) [+ add] )
 * The scale goes into the packed weights, the shift / residual add / ReLU into the store of the convolution kernel: the layer
 * is one launch and the un-normalised convolution result never reaches HBM.  All pointers are device pointers; `add` (same
 * shape as the output) may be NULL.  The struct itself lives in host memory and is read during the call. */
typedef struct mode_bn_epilogue {
  const float* gamma; /* (Co) BatchNorm weight */
  const float* beta;  /* (Co) BatchNorm bias */
  const float* mean;  /* (Co) running_mean */
  const float* var;   /* (Co) running_var */
  float eps;
  const float* add; /* residual added before the ReLU, or NULL */
  int relu;
} mode_bn_epilogue;

/* Version / diagnostics. */
#define MODE_HIP_ABI_VERSION 31 /* bumped whenever a signature below changes */
int mode_hip_abi_version(void);
const char* mode_last_error(void);

/* Test utility, not part of the operator seam (no reference counterpart): fills the LDS of every CU and the vector / accumulator
 * register files with `pattern`, on `stream`.  A kernel whose output depends on LDS words or registers it never wrote gives
 * pattern-dependent results; tests/test_gpu_repeat.py runs every operator of the training step behind it. */
int mode_debug_poison(unsigned pattern, mode_stream_t stream);

/* Inference with fixed weights (no reference counterpart: the reference re-reads its weights on every call, test_disparity.py:136).
 * Every forward entry that takes a `wpack` workspace first launches a small kernel that repacks the weights (with the folded
 * BatchNorm scale) into it -- 113 launches, 0.65 ms of a 10.3 ms eval forward at one pair.  After mode_weight_pack_reuse(1) those
 * entries SKIP the repacking on the calling thread and use `wpack` as it is: the caller guarantees that it still holds what the same
 * entry wrote for the same weights, BatchNorm parameters and shapes (mode_hip.functional keeps such workspaces per layer and keys
 * them on the tensors' versions).  mode_weight_pack_reuse(0) restores the default.  Returns the previous setting. */
int mode_weight_pack_reuse(int on);

/* ---------------------------------------------------------------------------------------------
 * Spherical convolution.
 *
 * Replaces sphere_conv_forward_cuda (sphere_conv_cuda.cpp:129-210 = per-sample im2col kernel
 * sphere_conv_cuda_kernel.cu:195-262 + addmm_) with ONE fused launch: the bilinear gather writes
 * the column tile to LDS and the contraction over Ci*Kh*Kw runs on fp32 MFMA; no HBM column buffer.
 *
 *   x   (B, Ci, H, W)            pos (1, 2*Kh*Kw, H, W): channel 2k = row coordinate, 2k+1 = column
 *   w   (Co, Ci/groups, Kh, Kw)  coordinate of tap k, sampled at (h_out*sH, w_out*sW)
 *   y   (B, Co, Ho, Wo)          written (not accumulated)
 *
 * `wpack` is scratch for the MFMA-fragment-ordered copy of the weights, >= mode_sphere_conv_wpack_bytes().
 * padding / dilation only enter the output-size formula (sphere_conv.py:112-113), so the caller
 * passes Ho, Wo.
 */
size_t mode_sphere_conv_wpack_bytes(int Ci, int Co, int Kh, int Kw, int groups);

int mode_sphere_conv_fwd(const float* x, const float* pos, const float* w, float* y, float* wpack,
                         int B, int Ci, int H, int W, int Co, int Kh, int Kw, int sH, int sW,
                         int Ho, int Wo, int groups, mode_stream_t stream);

/* sphereConvbn (models/submodule.py:61-74) -- and, through an integer table, any other convbn -- in eval mode as one launch:
 * mode_sphere_conv_fwd with the folded-BatchNorm epilogue (mode_bn_epilogue above). */
int mode_sphere_conv_fwd_bn(const float* x, const float* pos, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack,
                            int B, int Ci, int H, int W, int Co, int Kh, int Kw, int sH, int sW, int Ho, int Wo, int groups,
                            mode_stream_t stream);

/* Replaces the grad_input half of sphere_conv_backward_cuda (sphere_conv_cuda.cpp:275-294:
 * addmm_(W^T, gO) + col2im kernel sphere_conv_cuda_kernel.cu:293-356).  ACCUMULATES into gx, which
 * the caller zero-fills first, exactly like the reference (sphere_conv.py:62). */
int mode_sphere_conv_bwd_data(const float* gy, const float* pos, const float* w, float* gx, float* wpack,
                              int B, int Ci, int H, int W, int Co, int Kh, int Kw, int sH, int sW,
                              int Ho, int Wo, int groups, mode_stream_t stream);

/* The same gradient in gather form: deterministic, no atomics, ~7x faster.  It needs the ADJOINT of the sampling table,
 * which depends on the table only (a constant of the module, sphere_conv.py:150) and is built once on the HOST:
 *   mode_sphere_adjoint_build(pos_host, ...) fills rowptr_host[Kh*Kw*H*W + 1] and entries_host[2 * n] (n <=
 *   mode_sphere_adjoint_max_entries()) -- for tap k and input pixel q, entries rowptr[k*H*W+q] .. rowptr[k*H*W+q+1] are
 *   (output pixel p, float bits of the bilinear weight) pairs.  The caller uploads both arrays and passes the device
 *   copies to mode_sphere_conv_bwd_data_adj, which adds to gx like the scatter form (accumulate = 1) or overwrites it
 *   (accumulate = 0: no zero-fill and no read of gx needed). */
size_t mode_sphere_adjoint_max_entries(int Kh, int Kw, int Ho, int Wo);

int mode_sphere_adjoint_build(const float* pos_host, int H, int W, int Kh, int Kw, int sH, int sW, int Ho, int Wo,
                              int32_t* rowptr_host, int32_t* entries_host, int64_t* n_entries);

int mode_sphere_conv_bwd_data_adj(const float* gy, const float* w, float* gx, float* wpack, const int32_t* adj_rowptr,
                                  const int32_t* adj_entries, int B, int Ci, int H, int W, int Co, int Kh, int Kw,
                                  int Ho, int Wo, int groups, int accumulate, mode_stream_t stream);

/* The gather form restricted to a LIST of 64-pixel tiles of gx (tile t = linear pixels 64 t .. 64 t + 63 of the H x W image as it is
 * stored; n_list tiles per sample; 3x3 kernels): everything outside the list is left untouched. */
int mode_sphere_conv_bwd_data_adj_list(const float* gy, const float* w, float* gx, float* wpack, const int32_t* adj_rowptr,
                                       const int32_t* adj_entries, int B, int Ci, int H, int W, int Co, int Kh, int Kw,
                                       int Ho, int Wo, int groups, int accumulate, const int32_t* tile_list, int n_list,
                                       mode_stream_t stream);

/* Windowed input gradient on the split-bf16 matrix path (csrc/sphere_win_bwd_data.hip; replaces the col2im scatter of
 * sphere_conv_cuda_kernel.cu:293-356 + the GEMM of sphere_conv_cuda.cpp:275-315 for stride 1, 3x3 taps, output grid = input grid).
 * Host planning, once per table: mode_sphere_adjplan_build(pos_host, H, W, Kh, Kw, good_tiles[4 n], bad_tiles[2 n], counts[2],
 *   rec_off_host[n * 9 * 256 * 4], rec_w_host[same], rec_off2_host[n * 9 * 256 * 2], rec_w2_host[same]) with n =
 *   mode_sphere_plan_max_tiles(H, W): for every 64 x 4 tile of INPUT pixels whose adjoint lists all have <= 6 entries, with weights
 *   that sum to <= 65504 / 2^15 = 2 - 2^-10 per list (the plan's promise to the fp16 entry below), inside one 81-row
 *   x 8-column window of gy it writes (h0, w0, rbase, cbase | six << 16) and, per (tile, tap, pixel), 4 (window offset, weight) slots
 *   + 2 more in the second pair of arrays (six = 1 when any list of the tile uses them); the other tiles go to bad_tiles as (h0, w0).
 *   counts = (good, bad).  A tile that fails the weight sum alone is bad, and its entry (bit 17 of the fourth word set) and records follow
 *   those of the good tiles: mode_sphere_conv_bwd_data_win_split (three bf16 pieces, no headroom to keep) may run them once the bit is
 *   cleared and they are taken off the bad list; the fp16 entry must not.
 * mode_sphere_conv_bwd_data_win_split WRITES gx on the good tiles (fp32 operands split exactly into 3 bf16 pieces, 6 bf16 MFMAs per
 *   product, fp32 accumulation); the caller runs mode_sphere_conv_bwd_data_adj_list (accumulate = 0) on the bad ones.  `transposed`: gy
 *   and gx are plane-transposed (B, C, W, H).  Needs mode_sphere_conv_bwd_data_win_supported(Ci, Co, groups) == 1 (output channels per
 *   group a multiple of 16); `wpack` >= mode_sphere_conv_bwd_data_win_wpack_bytes(). */
int mode_sphere_adjplan_build(const float* pos_host, int H, int W, int Kh, int Kw, int32_t* good_tiles, int32_t* bad_tiles,
                              int32_t* counts, int32_t* rec_off_host, float* rec_w_host, int32_t* rec_off2_host, float* rec_w2_host);

size_t mode_sphere_conv_bwd_data_win_wpack_bytes(int Ci, int Co, int Kh, int Kw, int groups);

int mode_sphere_conv_bwd_data_win_supported(int Ci, int Co, int groups);

int mode_sphere_conv_bwd_data_win_split(const float* gy, const float* w, float* gx, float* wpack, const int32_t* tiles, int n_tiles,
                                        const int32_t* rec_off, const float* rec_w, const int32_t* rec_off2, const float* rec_w2, int B,
                                        int Ci, int H, int W, int Co, int Kh, int Kw, int groups, int transposed, mode_stream_t stream);
/* The same on the two-piece fp16 arithmetic of mode_sphere_conv_fwd_win_split_f16 (a backward pass is a training step): amax_g / amax_w =
 * the maximum buffers (MODE_BN_ABSMAX_FLOATS floats; mode_abs_max, mode_bn_train_bwd_amax) of gy and of w.  The operand it splits is
 * the adjoint-sampled gradient scaled by f16_scale_of(max |gy|): at most (a list's weight sum) x 2^15.  It is a finite fp16 number for
 * ANY gy because the plan holds every list of a good tile to a sum <= 2 - 2^-10; records from another source must keep that too. */
int mode_sphere_conv_bwd_data_win_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, float* gx, float* wpack,
                                            const int32_t* tiles, int n_tiles, const int32_t* rec_off, const float* rec_w,
                                            const int32_t* rec_off2, const float* rec_w2, int B, int Ci, int H, int W, int Co, int Kh,
                                            int Kw, int groups, int transposed, mode_stream_t stream);

/* Windowed forward (csrc/sphere_win_fwd.hip): same result as mode_sphere_conv_fwd for stride 1 and 3x3 taps, ~2x faster on
 * tables whose samples are spatially compact (the gnomonic tables of the network).  The caller plans the table once on the HOST
 * (the mode_sphere_*plan* entries: csrc/sphere_plan.hip, host code only):
 *   mode_sphere_plan_build(pos_host, ...) fills tiles_host[4 * mode_sphere_plan_max_tiles(H, W)] with (h0, w0, rbase, cbase)
 *   per 64x4 tile of output pixels (the window class is packed into bits 16.. of the 4th word) and counts[4] = tiles per
 *   class (81-row window, 145-row window, whole-axis window, does-not-fit).  If counts[3] != 0 the table is not compact: use mode_sphere_conv_fwd.
 * Otherwise upload the tile list and pass it with counts[0..2]; `wpack` >= mode_sphere_conv_win_wpack_bytes(). */
size_t mode_sphere_plan_max_tiles(int H, int W);

int mode_sphere_plan_build(const float* pos_host, int H, int W, int Kh, int Kw, int32_t* tiles_host, int32_t* counts);

size_t mode_sphere_conv_win_wpack_bytes(int Ci, int Co, int Kh, int Kw, int groups);

int mode_sphere_conv_fwd_win(const float* x, const float* pos, const float* w, float* y, float* wpack, const int32_t* tiles,
                             int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W, int Co, int Kh, int Kw,
                             int groups, int transposed, mode_stream_t stream);

int mode_sphere_conv_fwd_win_bn(const float* x, const float* pos, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack,
                                const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W, int Co, int Kh,
                                int Kw, int groups, int transposed, mode_stream_t stream);
/* The same call with the small-window tiles on the split-bf16 matrix path (needs Ci / groups % 16 == 0, else it is the
 * call above); bn may be NULL (plain convolution). */
int mode_sphere_conv_fwd_win_split(const float* x, const float* pos, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack,
                                const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W, int Co, int Kh,
                                int Kw, int groups, int transposed, mode_stream_t stream);

/* The plain (no epilogue) call of a TRAINING step with the small-window tiles on the two-piece fp16 arithmetic of the stride-1 3-D layers
 * (two fp16 pieces per value, three MFMAs per product, a power-of-two scale per operand): amax_x / amax_w = device scalars
 * holding the largest finite magnitude of x and of w (mode_abs_max, or mode_bn_train_fwd_amax of the pass that wrote x).
 * Ci / groups % 16 != 0: the call above with bn = NULL. */
int mode_sphere_conv_fwd_win_split_f16(const float* x, const float* pos, const float* w, const float* amax_x, const float* amax_w, float* y,
                                       float* wpack, const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W,
                                       int Co, int Kh, int Kw, int groups, int transposed, mode_stream_t stream);

/* `transposed` != 0: x and y are stored plane-transposed, (B, C, W, H) contiguous, i.e. with the h axis contiguous
 * (mode_transpose_planes converts).  For the Cassini tables of the network h is the shift-invariant longitude axis, and in
 * this storage every global access of the windowed kernels is a full contiguous segment.  H, W, the table and the plan
 * always refer to the logical (untransposed) image. */
int mode_transpose_planes(const float* in, float* out, long long planes, int H, int W, mode_stream_t stream);

/* Windowed weight gradient: the 81-row-window tiles of the plan run on the LDS-window kernel; the other tiles on the polar
 * kernel (mode_sphere_plan_polar; pass n_rest_pixels = 0 then) or, if they could not be planned, their pixels
 * (mode_sphere_plan_rest_pixels: linear indices h*W + w, sorted; at most H*W; n_polar_items = 0 then) on the general kernels.  ADDS to gw like
 * mode_sphere_conv_bwd_weight; deterministic.  `workspace` >= mode_sphere_conv_bwd_weight_win_workspace_bytes().
 * gy_t / x_t (both or neither): plane-transposed copies of gy / x for the windowed kernel (see mode_transpose_planes); the
 * general kernels always read gy / x (which may be null when gy_t / x_t are given and n_rest_pixels = 0). */
int mode_sphere_plan_rest_pixels(const int32_t* tiles_host, const int32_t* counts, int H, int W, int32_t* pix_host,
                                 int32_t* n_pix);

/* Sampling records of the 81-row-window tiles (window offset + 4 corner weights per tap and pixel), which the windowed
 * weight-gradient kernel reads instead of re-deriving them from the table: rec_w_host[4 * n], rec_off_host[n],
 * n = mode_sphere_plan_records_count(counts[0]).  Built once per table on the host, uploaded by the caller. */
size_t mode_sphere_plan_records_count(int n_small);

int mode_sphere_plan_records(const float* pos_host, const int32_t* tiles_host, const int32_t* counts, int H, int W,
                             float* rec_w_host, int32_t* rec_off_host);

/* Column items of the tiles that are not of the 81-row class, for the polar weight-gradient kernel (one output column of 32 pixels
 * per item, nine per-tap windows of 34 rows x 2 columns): pitems_host[20 * n], rec_w_host[4 * 288 * n], rec_off_host[288 * n],
 * n <= mode_sphere_plan_polar_max_items(counts); *n_items = -1 when some column does not fit (use the pixel list instead). */
size_t mode_sphere_plan_polar_max_items(const int32_t* counts);

int mode_sphere_plan_polar(const float* pos_host, const int32_t* tiles_host, const int32_t* counts, int H, int W,
                           int32_t* pitems_host, float* rec_w_host, int32_t* rec_off_host, int32_t* n_items);

size_t mode_sphere_conv_bwd_weight_win_workspace_bytes(int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups,
                                                       int n_small, int n_rest_pixels, int n_polar_items);

/* mode_sphere_conv_bwd_weight_win_split: the same call with the compact-window tiles on the split-bf16 kernel (K = 16 pixels per
 * v_mfma_f32_32x32x16_bf16, fp32 operands split exactly into three bf16 pieces, fp32 accumulation). */
int mode_sphere_conv_bwd_weight_win_split(const float* gy, const float* pos, const float* x, float* gw, float* workspace,
                                          const int32_t* tiles, int n_small, int n_mid, int n_wrap, const float* rec_w,
                                          const int32_t* rec_off, const int32_t* rest_pixels, int n_rest_pixels,
                                          const int32_t* pitems, const float* prec_w, const int32_t* prec_off, int n_polar_items,
                                          int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const float* gy_t,
                                          const float* x_t, mode_stream_t stream);

/* ... and with those tiles on the two-piece fp16 arithmetic of mode_sphere_conv_fwd_win_split_f16: amax_g / amax_x = the maximum buffers
 * (MODE_BN_ABSMAX_FLOATS floats) of gy and of x.  The polar items keep three bf16 pieces. */
int mode_sphere_conv_bwd_weight_win_split_f16(const float* gy, const float* pos, const float* x, const float* amax_g, const float* amax_x,
                                              float* gw, float* workspace, const int32_t* tiles, int n_small, int n_mid, int n_wrap,
                                              const float* rec_w, const int32_t* rec_off, const int32_t* rest_pixels, int n_rest_pixels,
                                              const int32_t* pitems, const float* prec_w, const int32_t* prec_off, int n_polar_items,
                                              int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const float* gy_t,
                                              const float* x_t, mode_stream_t stream);

int mode_sphere_conv_bwd_weight_win(const float* gy, const float* pos, const float* x, float* gw, float* workspace,
                                    const int32_t* tiles, int n_small, int n_mid, int n_wrap, const float* rec_w,
                                    const int32_t* rec_off, const int32_t* rest_pixels, int n_rest_pixels, const int32_t* pitems,
                                    const float* prec_w, const int32_t* prec_off, int n_polar_items, int B, int Ci, int H, int W,
                                    int Co, int Kh, int Kw, int groups, const float* gy_t, const float* x_t, mode_stream_t stream);

/* Replaces the grad_weight half (sphere_conv_cuda.cpp:296-315: second im2col + addmm_(gO, col^T),
 * summed over the batch).  ACCUMULATES into gw (caller zero-fills, sphere_conv.py:63).  `workspace`
 * holds the deterministic split-K partial sums: >= mode_sphere_conv_bwd_weight_workspace_bytes(). */
size_t mode_sphere_conv_bwd_weight_workspace_bytes(int B, int Ci, int Co, int Kh, int Kw, int Ho, int Wo,
                                                   int groups);

int mode_sphere_conv_bwd_weight(const float* gy, const float* pos, const float* x, float* gw, float* workspace,
                                int B, int Ci, int H, int W, int Co, int Kh, int Kw, int sH, int sW,
                                int Ho, int Wo, int groups, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Concatenation cost volume -- replaces the Python loop models/mode_disparity.py:104-113
 * (host-side zero tensor + H2D copy + 2*D4 strided slice copies + .contiguous()).
 *
 *   ref, tgt (B, C, H, W)  ->  cost (B, 2C, D4, H, W):
 *   cost[b, c, i, h, w] = ref[b, c, h, w], cost[b, C+c, i, h, w] = tgt[b, c, h, w-i] for w >= i, else 0.
 * Every output element is written exactly once (no memset).
 */
int mode_cost_volume_fwd(const float* ref, const float* tgt, float* cost, int B, int C, int D4, int H, int W,
                         mode_stream_t stream);

/* Autograd of the loop above: g_ref[b,c,h,w] = sum_{i<=w} g[b,c,i,h,w];
 * g_tgt[b,c,h,w] = sum_{i<W-w} g[b,C+c,i,h,w+i].  Writes (does not accumulate). */
int mode_cost_volume_bwd(const float* gcost, float* g_ref, float* g_tgt, int B, int C, int D4, int H, int W,
                         mode_stream_t stream);

/* Cost volume + first 3-D convolution without the volume (models/mode_disparity.py:104-116: the concatenation volume followed
 * by dres0[0][0] = Conv3d(2C -> Co, k3 s1 p1, no bias)).  The host forms the 18 partial products over (channel, kh)
 *   R[b, t*Co + o, h, w] = sum_{c,kh} W[o, c,   kd, kh, kw] * ref[b, c, h+kh-1, w],   t = kd*3 + kw,
 *   T[b, t*Co + o, h, u] = sum_{c,kh} W[o, C+c, kd, kh, kw] * tgt[b, c, h+kh-1, u]     (two GEMMs with K = 3C), and
 *   out[b,o,d,h,w] = sum_t [0 <= d' < D][d' <= w' < W] (R_t[b,o,h,w'] + T_t[b,o,h,w'-d']),  d' = d+kd-1, w' = w+kw-1
 * is the layer's output exactly (csrc/cost_conv.hip).  _bwd is the adjoint: gR, gT (B, 9*Co, H, W) from gout (B,Co,D,H,W);
 * both write (do not accumulate) and are deterministic. */
int mode_cost_conv_assemble_fwd(const float* R, const float* T, float* out, int B, int Co, int D, int H, int W, mode_stream_t stream);
int mode_cost_conv_assemble_bwd(const float* gout, float* gR, float* gT, int B, int Co, int D, int H, int W, mode_stream_t stream);

/* dres0[0] = convbn_3d(64, 32) + ReLU on the cost volume in eval mode: the assembly with the BatchNorm scale / shift (+ ReLU)
 * applied on the way out (bn->add must be NULL). */
int mode_cost_conv_assemble_fwd_bn(const float* R, const float* T, const mode_bn_epilogue* bn, float* out, int B, int Co, int D,
                                   int H, int W, mode_stream_t stream);
/* ... and (ABI 31) the maximum buffer of `out` filled on the way (MODE_BN_ABSMAX_FLOATS floats, zeroed by the call; NULL = the plain call):
 * the operand maximum of the next layer when it runs on the fp16 arithmetic in eval mode (mode_conv3d_fwd_split_f16_bn). */
int mode_cost_conv_assemble_fwd_bn_amax(const float* R, const float* T, const mode_bn_epilogue* bn, float* out, float* out_absmax, int B,
                                        int Co, int D, int H, int W, mode_stream_t stream);

/* Weight gradient of the regular 3x3 Conv2d layers of the extractor (nn.Conv2d inside convbn, models/submodule.py:15-17):
 * stride 1, padding = dilation in {1, 2}, no bias, groups 1.  gw (Co, Ci, 3, 3) (+)= sum_{b,h,w} gy[b,o,h,w] * x[b,c,h+(kh-1)*dil,
 * w+(kw-1)*dil]; gy (B,Co,H,W), x (B,Ci,H,W).  Deterministic.  `workspace` >= mode_conv2d_bwd_weight_workspace_bytes().
 * (Forward and input gradient of these layers stay on the vendor library's fp32 Winograd kernels.) */
/* Forward and input gradient of the same layers (used where they beat the vendor's Winograd: quarter resolution and dilation 2).
 * x (B,Ci,H,W), w (Co,Ci,3,3), y (B,Co,H,W); Co <= 128 (Ci <= 128 for _bwd_data).  Both overwrite their output.
 * `wpack` >= mode_conv2d_wpack_bytes(Ci, Co) bytes of scratch (fragment-ordered weights, rebuilt on every call). */
size_t mode_conv2d_wpack_bytes(int Ci, int Co);
int mode_conv2d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                    mode_stream_t stream);
int mode_conv2d_bwd_data(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                         mode_stream_t stream);

/* convbn (models/submodule.py:15-17) in eval mode as one launch: mode_conv2d_fwd with the folded-BatchNorm epilogue. */
int mode_conv2d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H,
                       int W, int Co, int dilation, mode_stream_t stream);

/* out (planes, 2*Ho, 2*Wo): out[p][2h][2w] = in[p][h][w], zero elsewhere (Wo even).  The gradients of the extractor's one
 * stride-2 3x3 layer (models/submodule.py:158) are the stride-1 gradients of the zero-inserted output gradient. */
int mode_zero_insert2(const float* in, float* out, long long planes, int Ho, int Wo, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 1x1 convolutions of the extractor (nn.Conv2d(kernel_size=1), models/submodule.py:162, 167-174: the `downsample` branches and
 * lastconv[0] / lastconv[4]; stride 1 or 2, no bias) as plain MFMA GEMMs over the NCHW planes -- csrc/conv1x1.hip.
 *   x (B, Ci, H, W)   w (Co, Ci[, 1, 1])   y (B, Co, Ho, Wo),  Ho = (H - 1) / stride + 1
 *   bwd_data WRITES gx (zeros where a stride-2 layer never read); bwd_weight writes gw (accumulate = 0) or adds to it, needs
 *   Wo % 4 == 0 (stride 2: W % 8 == 0) and `workspace` >= mode_conv1x1_bwd_weight_workspace_bytes().  Deterministic. */
size_t mode_conv1x1_wpack_bytes(int Ci, int Co);

int mode_conv1x1_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int H, int W, int Co, int stride,
                     mode_stream_t stream);

int mode_conv1x1_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H,
                        int W, int Co, int stride, mode_stream_t stream);

int mode_conv1x1_bwd_data(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int H, int W, int Co, int stride,
                          mode_stream_t stream);

size_t mode_conv1x1_bwd_weight_workspace_bytes(int B, int Ci, int H, int W, int Co, int stride);

int mode_conv1x1_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                            int stride, int accumulate, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The stem of the extractor: Conv2d(3 -> 32, kernel 7, stride 2, padding 3, no bias) on the full-resolution image
 * (firstconv[0], models/submodule.py:155) -- csrc/conv_stem.hip.  The image carries no gradient: forward and weight gradient only.
 *   x (B, 3, H, W)   w (Co <= 32, 3, 7, 7)   y (B, Co, Ho, Wo),  Ho = (H - 1) / 2 + 1
 *   bwd_weight writes gw (accumulate = 0) or adds to it; `workspace` >= mode_conv_stem_bwd_weight_workspace_bytes().  Deterministic. */
size_t mode_conv_stem_wpack_bytes(int Ci, int Co);

int mode_conv_stem_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int H, int W, int Co, mode_stream_t stream);

int mode_conv_stem_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H,
                          int W, int Co, mode_stream_t stream);

size_t mode_conv_stem_bwd_weight_workspace_bytes(int B, int Ci, int H, int W, int Co);

int mode_conv_stem_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                              int accumulate, mode_stream_t stream);
size_t mode_conv2d_bwd_weight_workspace_bytes(int B, int Ci, int H, int W, int Co);
int mode_conv2d_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                           int dilation, int accumulate, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3x3 convolution, padding 1, no bias -- replaces the cuDNN nn.Conv3d inside convbn_3d
 * (models/submodule.py:20-22) for dres0/dres1, the hourglass stride-1 layers and the classifier bodies
 * (models/mode_disparity.py:15-25, 66-80).  NCDHW fp32, implicit GEMM on fp32 MFMA.
 *
 *   x (B, Ci, D, H, W)   w (Co, Ci, 3, 3, 3)   y (B, Co, Do, Ho, Wo),  Xo = (X - 1) / stride + 1,  stride 1 or 2,
 *   Co and Ci <= 64 per call.  `wpack` >= mode_conv3d_wpack_bytes(Ci, Co) holds the fragment-ordered weights (rebuilt
 *   every call).  bwd_data writes gx (no accumulation; stride 2 needs even D, H, W); bwd_weight writes gw
 *   (accumulate = 0) or adds to it (accumulate = 1) using `workspace` >= mode_conv3d_bwd_weight_workspace_bytes() for
 *   deterministic split-K partial sums.
 *
 * mode_deconv3d_fwd: ConvTranspose3d k3 s2 p1 op1, no bias (hourglass conv5/conv6, models/mode_disparity.py:23, 25):
 *   x (B, Cin, D, H, W)   w (Cin, Cout, 3, 3, 3)   y (B, Cout, 2D, 2H, 2W).
 *   Its backward-data is mode_conv3d_fwd(gy, w, ..., Ci = Cout, Co = Cin, stride = 2) (same memory layout) and its
 *   backward-weight is mode_conv3d_bwd_weight(gy := x, x := gy_out, Ci = Cout, Co = Cin, stride = 2).
 */
size_t mode_conv3d_wpack_bytes(int Ci, int Co);

int mode_conv3d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Ci, int D, int H, int W, int Co,
                    int stride, mode_stream_t stream);

int mode_conv3d_bwd_data(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W,
                         int Co, int stride, mode_stream_t stream);

/* convbn_3d in eval mode as ONE launch (+ the weight packing): mode_conv3d_fwd / mode_deconv3d_fwd with the folded-BatchNorm
 * epilogue above (Co > 1). */
int mode_conv3d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int D,
                       int H, int W, int Co, int stride, mode_stream_t stream);

int mode_deconv3d_fwd_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Cin, int D,
                         int H, int W, int Cout, mode_stream_t stream);

/* The same stride-1 layers on the bf16 matrix pipe with three-way split fp32 operands (csrc/conv3d_split.hip): six exact bf16
 * partial products per fp32 product, fp32 accumulation -- the rounding of an fp32 convolution at ~1.7 x the speed of the fp32 MFMA
 * kernels.  mode_conv3d_split_supported() says whether a layer can take this path (stride 1, <= 64 output channels of the GEMM,
 * reduction channels a multiple of 8; in the input-gradient GEMM the roles of Ci / Co are swapped; weight gradient: stride 1 and
 * more than one output channel).  mode_conv3d_fwd_split takes an optional folded-BatchNorm epilogue (NULL: plain convolution);
 * wpack as mode_conv3d_fwd; mode_conv3d_bwd_weight_split: arguments and workspace as mode_conv3d_bwd_weight with stride 1. */
int mode_conv3d_split_supported(int Ci, int Co, int stride, int which /* 0 forward, 1 input gradient, 2 weight gradient */);
/* Host only, launches nothing.  1 exactly when mode_conv3d_split_supported(Ci, Co, stride, which) == 1 AND the volume is inside every
 * 32-bit contract of the split kernel that the corresponding entry launches (descriptor sizes and lane offsets of its buffer loads,
 * element offsets of its epilogue; even sizes / W % 8 where the stride-2 entries need them; csrc/size_contracts.h has the derivations).
 * (Ci, Co, D, H, W, stride) describe the CONVOLUTION x (Ci, D, H, W) -> y (Co, D / stride, ...) whichever of its GEMMs `which` names; a
 * transposed convolution (Cin, d, h, w) -> (Cout, 2d, 2h, 2w) asks (Cout, Cin, 2d, 2h, 2w, 2, 1).  Every split entry below refuses
 * (MODE_ERR_UNSUPPORTED, before it looks at a pointer) exactly where this says 0: a caller falls back to the fp32 entries there. */
int mode_conv3d_split_shape_supported(int Ci, int Co, int D, int H, int W, int stride, int which);
/* Stride-2 forward (k3 p1) on the split-bf16 kernel (csrc/conv3d_split_s2.hip): hourglass conv1 / conv3 (mode_disparity.py:17-19) and
 * the input gradient of the transposed convolutions conv5 / conv6 (w = their (Cin, Cout, 27) weight read as (Co = Cin, Ci = Cout));
 * 33..64 output channels, input channels a multiple of 8: mode_conv3d_split_supported(Ci, Co, 2, 0) == 1.  bn: optional folded
 * eval-mode BatchNorm (+ residual) (+ ReLU) epilogue as in mode_conv3d_fwd_split. */
int mode_conv3d_fwd_s2_split(const float* x, const float* w, const mode_bn_epilogue* bn /* optional: eval-mode fold, NULL = plain */,
                             float* y, float* wpack, int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream);
/* (ABI 31) the same with the maximum buffer of y out of the eval epilogue (out_absmax: MODE_BN_ABSMAX_FLOATS floats, zeroed by the call;
 * needs bn; NULL = the plain call) -- see mode_conv3d_fwd_split_f16_bn. */
int mode_conv3d_fwd_s2_split_amax(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* out_absmax, float* wpack, int B,
                                  int Ci, int D, int H, int W, int Co, mode_stream_t stream);

/* The transposed convolution (ConvTranspose3d k3 s2 p1 op1, hourglass conv5 / conv6, mode_disparity.py:23-25) and the input gradient
 * of the stride-2 convolution -- one operator -- on the split-bf16 kernel of csrc/conv3d_split_deconv.hip: input channels of the
 * transposed convolution a multiple of 8, 2..64 output channels (mode_deconv3d_split_supported(Cin, Cout) /
 * mode_conv3d_split_supported(Ci, Co, 2, 1)); even D, H, W for the gradient form. */
int mode_deconv3d_split_supported(int Cin, int Cout);
int mode_deconv3d_fwd_split(const float* x, const float* w, float* y, float* wpack, int B, int Cin, int D, int H, int W, int Cout,
                            mode_stream_t stream);
/* The same with the folded eval-mode BatchNorm (+ residual) (+ ReLU) epilogue of mode_deconv3d_fwd_bn (convbn_3d around the
 * ConvTranspose3d of hourglass conv5 / conv6 in eval mode, mode_disparity.py:23-25, 38-45): whole 32-channel output tiles
 * (mode_deconv3d_split_bn_supported(Cin, Cout) == 1); wpack >= mode_conv3d_wpack_bytes(Cin, Cout). */
/* The arithmetic of the stride-1 3x3x3 layers (nn.Conv3d of convbn_3d, models/submodule.py:20-22) in a training step (the product
 * default since round 5, functional.CONV3D_S1_F16) AND, by default, in an inference forward (mode_conv3d_fwd_split_f16_bn below and
 * mode_conv2d_fwd_split_f16_bn; functional.CONV3D_EVAL_F16 / CONV2D_EVAL_F16.  Opting out: a caller of this interface calls the three-piece
 * entries, mode_conv3d_fwd_split / mode_conv2d_fwd_split with the epilogue; the Python layer sets those two module globals to False, which
 * is what `bench.py --no-eval-f16` does): fp32 operands split into TWO fp16 pieces, three v_mfma_f32_32x32x16_f16 per product
 * instead of six bf16 ones (2^-22 per product).  fp16's range is narrow, so each operand is scaled by a power of two that brings its
 * tensor's largest finite magnitude to [2^14, 2^15): amax_* = DEVICE buffers of MODE_BN_ABSMAX_FLOATS floats, one per operand (layout:
 * see MODE_BN_ABSMAX_FLOATS below), filled by mode_abs_max (an order-independent maximum over bit patterns; no host synchronisation,
 * graph-capturable) or by the `_amax` BatchNorm entries that write the tensor; a tensor's maximum can be computed once and passed to
 * every call that reads the tensor.  PRECISION CONTRACT: an element keeps 22 significant bits down to ~2^-17 of its tensor's maximum,
 * fewer below that, none below ~2^-39 of it (it contributes less than 2^-17 of the tensor's scale to any sum either way; the three-piece
 * bf16 entries keep 24 bits for every element) -- csrc/split_arith.h states both arithmetics and defines their primitives; DESIGN.md 3u.
 * mode_conv3d_bwd_data_split_f16: acc may be NULL.  mode_conv3d_bwd_weight_split_f16: other arguments and workspace as
 * mode_conv3d_bwd_weight_split. */
int mode_abs_max(const float* x, long long n, float* out_device_buffer, mode_stream_t stream);
/* The same for n tensors in ONE launch (one workgroup per tensor: meant for the tens of small WEIGHT tensors of a model, whose maxima a
 * training step needs before its first convolution): device_ptrs / device_sizes = DEVICE arrays of n tensor addresses / element counts,
 * out = n consecutive maximum buffers (n * MODE_BN_ABSMAX_FLOATS floats), all written. */
int mode_abs_max_batch(const float* const* device_ptrs, const long long* device_sizes, int n, float* out, mode_stream_t stream);
int mode_conv3d_fwd_split_f16(const float* x, const float* w, const float* amax_x, const float* amax_w, float* y, float* wpack, int B, int Ci,
                              int D, int H, int W, int Co, mode_stream_t stream);
int mode_conv3d_bwd_data_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, const float* acc, float* gx,
                                   float* wpack, int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream);
/* INFERENCE on the same arithmetic (ABI 31): y = relu?(bn(conv3d(x, w)) [+ bn->add]) as mode_conv3d_fwd_split with a non-NULL epilogue, on
 * two fp16 pieces.  The BatchNorm scale is folded into the weights before they are scaled and split: their maximum is the FOLDED weights',
 * taken inside the call where they are packed and kept in wpack (same size as for mode_conv3d_fwd_split; mode_pack_reuse applies to it as
 * to the packed weights).  In eval mode no BatchNorm pass writes the activations, so the kernel's epilogue leaves the maximum of what it
 * stored in amax_y (MODE_BN_ABSMAX_FLOATS floats, zeroed and filled by the call): the next layer's amax_x. */
int mode_conv3d_fwd_split_f16_bn(const float* x, const float* w, const float* amax_x, const mode_bn_epilogue* bn, float* y, float* amax_y,
                                 float* wpack, int B, int Ci, int D, int H, int W, int Co, mode_stream_t stream);
int mode_conv3d_bwd_weight_split_f16(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw, float* workspace,
                                     int B, int Ci, int D, int H, int W, int Co, int accumulate, mode_stream_t stream);
/* The input gradient of a stride-1 / stride-2 convolution on the split kernels with a gradient that is already there added in the
 * store: gx = conv^T(gy) + acc, bit for bit the sum autograd would form with a separate pass (x has a second consumer whose gradient
 * came first: a residual skip, a classifier head).  acc has gx's shape and must not alias it; stride 2: whole 32-channel tiles of gx
 * (mode_conv3d_bwd_data_split_acc_supported(Ci, Co, stride) == 1), even D, H, W. */
int mode_conv3d_bwd_data_split_acc_supported(int Ci, int Co, int stride);
int mode_conv3d_bwd_data_split_acc(const float* gy, const float* w, const float* acc, float* gx, float* wpack, int B, int Ci, int D, int H,
                                   int W, int Co, int stride, mode_stream_t stream);
int mode_deconv3d_split_bn_supported(int Cin, int Cout);
int mode_deconv3d_fwd_split_bn(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Cin, int D,
                               int H, int W, int Cout, mode_stream_t stream);
int mode_deconv3d_fwd_split_bn_amax(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* out_absmax /* as above */,
                                    float* wpack, int B, int Cin, int D, int H, int W, int Cout, mode_stream_t stream);
int mode_conv3d_bwd_data_s2_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W, int Co,
                                  mode_stream_t stream);
/* The weight gradient of the stride-2 convolution on the split-bf16 kernel of csrc/conv3d_split_wgrad_s2.hip (the gradients cuDNN
 * computes for hourglass conv1 / conv3, mode_disparity.py:17-19; called with gy := the input of a ConvTranspose3d and x := the gradient
 * of its output it gives that layer's (Cin, Cout, 27) weight gradient: conv5 / conv6, :23-25).  Arguments and workspace as
 * mode_conv3d_bwd_weight with stride 2; x channels a multiple of 32, gy channels a multiple of 64
 * (mode_conv3d_split_supported(Ci, Co, 2, 2) == 1), D and H even, W a multiple of 8. */
int mode_conv3d_bwd_weight_s2_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H, int W,
                                    int Co, int accumulate, mode_stream_t stream);

int mode_conv3d_fwd_split(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int D,
                          int H, int W, int Co, mode_stream_t stream);
int mode_conv3d_bwd_data_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int D, int H, int W, int Co,
                               mode_stream_t stream);
int mode_conv3d_bwd_weight_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H, int W,
                                 int Co, int accumulate, mode_stream_t stream);

/* The regular 3x3 Conv2d layers (stride 1, dilation 1 / 2) on the same split-bf16 path (csrc/conv2d_split.hip): reduction channels
 * a multiple of 16, <= 512 output channels of the GEMM (one launch per block of 64); arguments and wpack as mode_conv2d_fwd / _bwd_data
 * (+ optional epilogue). */
int mode_conv2d_split_supported(int Ci, int Co, int dilation, int which /* 0 forward, 1 input gradient */);
/* Host only, launches nothing: the same for an H x W image -- the layer is supported (which 2, the weight gradient: any channel counts)
 * AND the image is inside the 32-bit contracts of the split kernel of `which` (csrc/size_contracts.h).  The 3 x 3 weight gradient of a
 * layer of up to 32 channels ends just below 2048 x 4096 pixels. */
int mode_conv2d_split_shape_supported(int Ci, int Co, int H, int W, int dilation, int which /* 0, 1, 2 weight gradient */);
int mode_conv2d_fwd_split(const float* x, const float* w, const mode_bn_epilogue* bn, float* y, float* wpack, int B, int Ci, int H, int W,
                          int Co, int dilation, mode_stream_t stream);
int mode_conv2d_bwd_data_split(const float* gy, const float* w, float* gx, float* wpack, int B, int Ci, int H, int W, int Co, int dilation,
                               mode_stream_t stream);
/* The same with a gradient of the same tensor that is already there added in the store (gx = conv^T(gy) + acc, bit for bit autograd's
 * sum; acc has gx's shape and must not alias it): the input of a residual block of the extractor has two consumers, its first
 * convolution and the skip (models/submodule.py:36-46, 110-118).  Same predicate as mode_conv2d_bwd_data_split. */
int mode_conv2d_bwd_data_split_acc(const float* gy, const float* w, const float* acc, float* gx, float* wpack, int B, int Ci, int H, int W,
                                   int Co, int dilation, mode_stream_t stream);
/* mode_conv2d_fwd_split / mode_conv2d_bwd_data_split(_acc) of a TRAINING step on the two-piece fp16 arithmetic of the stride-1 3-D layers
 * (two fp16 pieces per value, three MFMAs per product, a power-of-two scale per operand): amax_* = the maximum buffers
 * (MODE_BN_ABSMAX_FLOATS floats: mode_abs_max, mode_bn_train_fwd_amax, mode_bn_train_bwd_amax) of the activation / gradient and of the
 * weight.  Same predicate (mode_conv2d_split_supported) and workspace; acc may be NULL. */
int mode_conv2d_fwd_split_f16(const float* x, const float* w, const float* amax_x, const float* amax_w, float* y, float* wpack, int B, int Ci,
                              int H, int W, int Co, int dilation, mode_stream_t stream);
int mode_conv2d_bwd_data_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, const float* acc, float* gx,
                                   float* wpack, int B, int Ci, int H, int W, int Co, int dilation, mode_stream_t stream);
/* INFERENCE on that arithmetic (ABI 31), the 2-D twin of mode_conv3d_fwd_split_f16_bn: mode_conv2d_fwd_split with a non-NULL epilogue on two
 * fp16 pieces; the folded weights' maximum is taken inside with the pack and kept in wpack (mode_conv2d_wpack_bytes has the room since
 * ABI 31), amax_x = the input's maximum buffer, amax_y = the stored output's (zeroed and filled by the call: the next layer's amax_x). */
int mode_conv2d_fwd_split_f16_bn(const float* x, const float* w, const float* amax_x, const mode_bn_epilogue* bn, float* y, float* amax_y,
                                 float* wpack, int B, int Ci, int H, int W, int Co, int dilation, mode_stream_t stream);
int mode_conv2d_bwd_weight_split(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int H, int W, int Co,
                                 int dilation, int accumulate, mode_stream_t stream);
/* ... on the two-piece fp16 arithmetic (mode_conv2d_fwd_split_f16): amax_g / amax_x = the maximum buffers of gy and of x. */
int mode_conv2d_bwd_weight_split_f16(const float* gy, const float* x, const float* amax_g, const float* amax_x, float* gw, float* workspace,
                                     int B, int Ci, int H, int W, int Co, int dilation, int accumulate, mode_stream_t stream); /* arguments / workspace: mode_conv2d_bwd_weight */

size_t mode_conv3d_bwd_weight_workspace_bytes(int B, int Ci, int D, int H, int W, int Co, int stride);

int mode_conv3d_bwd_weight(const float* gy, const float* x, float* gw, float* workspace, int B, int Ci, int D, int H,
                           int W, int Co, int stride, int accumulate, mode_stream_t stream);

int mode_deconv3d_fwd(const float* x, const float* w, float* y, float* wpack, int B, int Cin, int D, int H, int W,
                      int Cout, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused soft-argmin head -- replaces F.upsample(trilinear, align_corners=True) + F.softmax +
 * disparityregression (models/mode_disparity.py:131-152, models/submodule.py:50-57) and, when `conf` is non-NULL, the
 * confidence map of models/mode_disparity.py:157-183.  The (B,D,H,W) upsampled logits / probabilities are never
 * materialised.
 *
 *   logits (B, D4, H4, W4) [= the (B,1,D4,H4,W4) classifier output]  ->  pred (B, H, W) [, conf (B, H, W)]
 *   pred = sum_d d * softmax_d(upsample(logits))[d],   d = 0 .. D-1
 * mode_head_bwd: glogits (B,D4,H4,W4) = d(sum(gpred * pred)) / d logits, written (not accumulated); deterministic.
 * `workspace` >= mode_head_bwd_workspace_bytes(B, D4, H, W).
 */
int mode_head_fwd(const float* logits, float* pred, float* conf, int B, int D4, int H4, int W4, int D, int H, int W,
                  mode_stream_t stream);

size_t mode_head_bwd_workspace_bytes(int B, int D4, int H, int W);

int mode_head_bwd(const float* logits, const float* gpred, float* glogits, float* workspace, int B, int D4, int H4,
                  int W4, int D, int H, int W, mode_stream_t stream);

/* The head's backward with the gradient of the confidence map as well, in one pass over the pixels (same launches, same workspace
 * as mode_head_bwd): glogits = d(sum(gpred * pred) + sum(gconf * conf)) / d logits, written; deterministic.  pred, conf (B, H, W) are
 * the forward's own outputs of mode_head_fwd on the same logits: the gradient is that of the confidence that was reported.  With
 * p_d the softmax of the up-sampled column, r = rintf(pred), i_k = clamp(r + k, 0, D - 1) for k = -1, 0, 1 and m_d the number of k
 * with i_k == d (0 .. 3: at the borders an index counts twice, which is why conf can exceed 1), the value scattered to the two nodes
 * of disparity d is
 *   gv_d = p_d * (gpred * (d - pred) + gconf * (m_d - conf))
 * The rounding passes no gradient (the reference's grid_sample(mode='nearest') passes it to the probabilities alone).  With
 * gconf == 0 the result has the bits of mode_head_bwd.  Arguments are checked before any launch as mode_head_bwd checks them;
 * B = 0 is a no-op. */
int mode_head_bwd_conf(const float* logits, const float* pred, const float* conf, const float* gpred, const float* gconf,
                       float* glogits, float* workspace, int B, int D4, int H4, int W4, int D, int H, int W, mode_stream_t stream);

/* The loss of the training step next to the head (train_disparity.py:151-158: masked smooth-L1 of the three predictions, weights
 * 0.5 / 0.7 / 1.0, mean over the valid pixels), so that nothing elementwise is launched between the head and the optimizer:
 *   mode_smooth_l1_masked: out[0] = scale[0] * sum_i w_i * sum_pix [gt == gt] * smooth_l1(pred_i[pix] - gt[pix])   (beta = 1);
 *     pred1 / pred2 may be NULL; NaN ground truth = masked pixel (train_disparity.py:195); scale = a DEVICE scalar, normally
 *     1 / (number of valid pixels over all ranks); n = B * H * W; workspace >= mode_smooth_l1_workspace_bytes(n); deterministic.
 *   mode_head_bwd_loss: mode_head_bwd with gpred = weight * scale[0] * [gt == gt] * clamp(pred - gt, -1, 1) formed inside the kernel from
 *     the forward's own prediction `pred` (B, H, W) -- the gradient of the term weight * scale * sum smooth_l1(pred - gt) above; `scale`
 *     here also carries the upstream gradient of the loss.  workspace as mode_head_bwd.  Only where mode_head_loss_supported(...) == 1
 *     (D = 4 * D4 with D4 one of 4 / 8 / 12 / 16 / 48 / 64, W <= 512); otherwise form gpred and call mode_head_bwd.
 */
size_t mode_smooth_l1_workspace_bytes(long long n);

int mode_smooth_l1_masked(const float* pred0, const float* pred1, const float* pred2, const float* gt, float w0, float w1, float w2,
                          const float* scale, float* out, float* workspace, long long n, mode_stream_t stream);

int mode_head_loss_supported(int B, int D4, int H4, int W4, int D, int H, int W);

int mode_head_bwd_loss(const float* logits, const float* pred, const float* gt, float weight, const float* scale, float* glogits,
                       float* workspace, int B, int D4, int H4, int W4, int D, int H, int W, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm (+ residual add) (+ ReLU) over (B, C, S) tensors, S = D*H*W or H*W, S % 4 == 0.
 * Replaces nn.BatchNorm3d/2d of convbn_3d / convbn (models/submodule.py:15-22) fused with the adds and ReLUs that
 * follow it in hourglass.forward / ModeDisparity.forward (models/mode_disparity.py:27-46, 115-129):
 *      out = relu?( gamma * (y - mean) / sqrt(var + eps) + beta  [+ add] )
 * train: batch statistics over (B, S) per channel (biased variance for normalisation); running_mean / running_var are
 *        updated in place with `momentum` (unbiased variance) and *num_batches_tracked is incremented (either may be
 *        NULL), as nn.BatchNorm does; save_mean / save_invstd feed the backward.  Two launches.
 * eval : running statistics.  One launch.
 * bwd  : g = relu ? gout * (out > 0) : gout;  gy = dL/dy written; gadd (optional, = g) written if non-NULL;
 *        ggamma / gbeta written (accumulate = 0) or added to (accumulate = 1: the caller's gradient buffer, which saves
 *        the separate accumulation kernels of autograd).  Two launches.
 *        The ReLU mask comes from `out`; when no residual was added, `out` may be NULL and the mask is rebuilt bit-exactly
 *        from y with the float32 save_scale / save_shift (C floats each, optional outputs of the forward): one tensor less
 *        to read in both backward passes.
 * groups: statistics over `groups` consecutive sub-batches of B / groups samples each (1 = the whole batch) -- what `groups`
 *        consecutive calls of the module on the sub-batches would compute, including the order of the running-statistics
 *        updates; save_* hold groups * C values.  Used to run the left and right images through the shared extractor as one batch.
 * `workspace` >= mode_bn_workspace_bytes(C * groups) for the training calls.
 * mode_bn_train_fwd is NOT in-place: `out` must not alias `y` (the normalisation pass re-reads one element per channel of y -- the
 *        pivot of the shifted sums -- while it writes `out`); out == y returns MODE_ERR_BAD_ARG.  Nor is mode_bn_train_bwd, for the
 *        same reason (channels whose mean dominates, |mean| > 16 std, sum g * (y - pivot)): gy == y returns MODE_ERR_BAD_ARG.
 */
size_t mode_bn_workspace_bytes(int C);

int mode_bn_train_fwd(const float* y, const float* add, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu,
                      float* out, float* save_mean, float* save_invstd, float* save_scale, float* save_shift,
                      float* workspace, int B, int C, long long S, int groups, mode_stream_t stream);

/* A tensor's largest finite magnitude, as the fp16-arithmetic entries (mode_conv3d_*_split_f16, mode_sphere_conv_fwd_win_split_f16) take
 * it: a device buffer of MODE_BN_ABSMAX_FLOATS floats whose MAXIMUM is the value -- word 0 and 128 words of 128 different cache lines,
 * everything else zero (the blocks of the producing pass each add to one of them: one word for a whole launch serialises at the memory
 * side; the consumers' waves read all 129).  mode_abs_max fills such a buffer with a pass over the tensor; the `_amax` entries below fill
 * one on the way -- the operand maximum comes out of the pass that WRITES the tensor: mode_bn_train_fwd_amax (+ _prestats_amax) for `out`,
 * mode_bn_train_bwd_amax and mode_classif_train_bwd_amax for the gradient `gy` (read by both gradients of the convolution in front).
 * Same arguments as the plain entries plus the buffer (NULL = the plain call); the call zeroes the whole buffer first.  (ABI <= 29 had
 * one-shot thread-local setters, mode_bn_next_out_absmax / mode_bn_next_gy_absmax, instead: removed.) */
#define MODE_BN_ABSMAX_FLOATS 2064
int mode_bn_train_fwd_amax(const float* y, const float* add, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu, float* out,
                           float* save_mean, float* save_invstd, float* save_scale, float* save_shift, float* workspace, int B, int C,
                           long long S, int groups, float* out_absmax, mode_stream_t stream);

int mode_bn_eval_fwd(const float* y, const float* add, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, int relu, float* out, int B, int C, long long S,
                     mode_stream_t stream);

int mode_bn_train_bwd(const float* gout, const float* y, const float* out, const float* gamma, const float* save_mean,
                      const float* save_invstd, const float* save_scale, const float* save_shift, int relu, float* gy,
                      float* gadd, float* ggamma, float* gbeta, int accumulate, float* workspace, int B, int C,
                      long long S, int groups, mode_stream_t stream);
int mode_bn_train_bwd_amax(const float* gout, const float* y, const float* out, const float* gamma, const float* save_mean,
                           const float* save_invstd, const float* save_scale, const float* save_shift, int relu, float* gy,
                           float* gadd, float* ggamma, float* gbeta, int accumulate, float* workspace, int B, int C,
                           long long S, int groups, float* gy_absmax, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Classifier head of the 3-D regulariser in TRAINING (SURVEY a12 + a15):
 *     classifN = Sequential(convbn_3d(32, 32), ReLU, Conv3d(32, 1, k3 p1, bias=False))      models/mode_disparity.py:76-80
 *     cost1 = classif1(out1); cost2 = classif2(out2) + cost1; cost3 = classif3(out3) + cost2  models/mode_disparity.py:127-129
 * taken from the OUTPUT y (B, C, D, H, W) of the first convolution on: BatchNorm3d (batch statistics, torch defaults as in
 * mode_bn_train_fwd) + ReLU + the single-channel convolution [+ the residual `add` (B, 1, D, H, W), may be NULL], without the
 * activated tensor relu(bn(y)) ever being written (csrc/classif_head.hip: the normalisation is applied while the second convolution
 * stages its operand; in the backward ONE pass over y yields the weight gradient of the second convolution and both reductions of the
 * BatchNorm backward, a second one its input gradient with the BatchNorm backward's apply pass in the store).  C <= 32.
 *   fwd: cost (B, 1, D, H, W) written; running_mean / running_var / *num_batches_tracked updated (any may be NULL);
 *        save_mean / save_invstd / save_scale / save_shift (C floats each) feed the backward.
 *   bwd: gcost (B, 1, D, H, W) = dL/dcost -> gy (B, C, D, H, W) = dL/dy written; gw (C * 27) = gradient of the second convolution's
 *        weight (1, C, 3, 3, 3), ggamma / gbeta (C): written (accumulate = 0) or added to (accumulate = 1).  The gradient of `add` is
 *        gcost itself.  Deterministic (fixed-order split-K).
 * `workspace` >= mode_classif_workspace_bytes(B, C, D, H, W), 16-byte aligned, for both calls.
 */
size_t mode_classif_workspace_bytes(int B, int C, int D, int H, int W);

int mode_classif_train_fwd(const float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           long long* num_batches_tracked, float momentum, float eps, const float* w, const float* add, float* cost,
                           float* save_mean, float* save_invstd, float* save_scale, float* save_shift, float* workspace, int B, int C,
                           int D, int H, int W, mode_stream_t stream);

int mode_classif_train_bwd(const float* gcost, const float* y, const float* w, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, const float* save_scale, const float* save_shift, float* gy,
                           float* gw, float* ggamma, float* gbeta, int accumulate, float* workspace, int B, int C, int D, int H, int W,
                           mode_stream_t stream);
int mode_classif_train_bwd_amax(const float* gcost, const float* y, const float* w, const float* gamma, const float* beta,
                                const float* save_mean, const float* save_invstd, const float* save_scale, const float* save_shift,
                                float* gy, float* gw, float* ggamma, float* gbeta, int accumulate, float* workspace, int B, int C, int D,
                                int H, int W, float* gy_absmax /* may be NULL */, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Export-stage geometry: what happens between the disparity network and the fusion network.
 *
 * mode_disp2depth: sine-rule depth of save_output_disparity_stage.py:105-135 for a Cassini disparity map (H, W);
 *   disp == 0 -> 1000, clamp to [0, 1000]; `baseline` = the camera-pair baseline.
 * mode_grid_sample_border: F.grid_sample(bilinear, align_corners=True, padding_mode='border') as used by cassini2Equirec /
 *   rotateCassini / erp2rect_cassini (utils/geometry.py:38, 92, 188); src (N,C,Hs,Ws), grid (grids,Ho,Wo,2) with grids = 1
 *   (shared) or N, dst (N,C,Ho,Wo).
 * mode_depth_view_trans: depthViewTransWithConf (utils/geometry.py:99-145) including the sequential z-buffer of
 *   __iterPixels_with_conf (:148-156), reproduced bit-for-bit with a 64-bit atomic min.  view1/conf1/view2/conf2 (H, W);
 *   trig = the float32 values the reference computes with numpy, concatenated: sin phi[W], cos phi[W], sin theta[H],
 *   cos theta[H] (device array of 2W + 2H floats; the products r*sin(phi), (r*cos(phi))*sin(theta), (r*cos(phi))*cos(theta) are
 *   formed in that order like numpy's); R (9 doubles, row-major) and t (3 doubles) on the HOST;
 *   workspace >= mode_depth_view_trans_workspace_bytes.
 */
int mode_disp2depth(const float* disp, float* depth, int H, int W, float baseline, mode_stream_t stream);

int mode_grid_sample_border(const float* src, const float* grid, float* dst, int N, int C, int Hs, int Ws, int Ho, int Wo,
                            int grids, mode_stream_t stream);

size_t mode_depth_view_trans_workspace_bytes(int H, int W);

int mode_depth_view_trans(const float* view1, const float* conf1, const float* trig, const double* R, const double* t,
                          float* view2, float* conf2, void* workspace, int H, int W, mode_stream_t stream);

/* The two halves of mode_depth_view_trans on their own: the projection of every source pixel (r2 in float64, target index
 * i*W + j or -1), and the z-buffer over n given (r2, target) pairs (workspace >= 8 n bytes).  The z-buffer is exact; the
 * projection rounds angles to pixel indices, and the reference's maps put whole families of points exactly on the rounding
 * boundary, where the last bit of atan2 / asin decides -- parity of the projection is therefore tested off those boundaries. */
int mode_depth_view_project(const float* view1, const float* trig, const double* R, const double* t, double* r2, int32_t* target,
                            int H, int W, mode_stream_t stream);

int mode_zbuffer(const double* r2, const int32_t* target, const float* conf1, float* view2, float* conf2, void* workspace,
                 long long n, mode_stream_t stream);

/* Multi-view hand-off (csrc/multiview.hip): the six camera pairs (order 12, 13, 14, 23, 24, 34) of F Deep360 frames from the
 * disparity network to the fusion network in three launches.  disp, conf (F, 6, H, W) -> out (F, 12, H, W) with
 *   out[f, 2p] = depth, out[f, 2p + 1] = confidence   of what the single-map entries compute for pair p: mode_disp2depth (12);
 *                                                     + mode_grid_sample_border on [depth; conf] (13, 14); + mode_depth_view_trans (23, 24, 34)
 * bit for bit, or out (F, 6, H, W) with out[f, p] = depth under MODE_MV_DEPTH_ONLY.  MODE_MV_CONF_PNG rounds every confidence
 * as the reference's 8-bit PNG round trip does: q(c) = (float)((double)min(255, max(0, rint(c * 255.0f))) / 255.0) (half to even).
 *   baselines6  host, the baseline of every pair
 *   rot_grids   device (2, H, W, 2), 8-byte aligned: the rotateCassini grids of pitch pi/2 (13) and pi/4 (14)
 *   trig        device, as mode_depth_view_trans
 *   xforms      host, 3 x (R[9] row-major, t[3]) for pairs 23, 24, 34, as mode_depth_view_trans
 *   workspace   device, 8-byte aligned, >= mode_multiview_handoff_workspace_bytes(F, H, W) = 3 F H W 8 bytes (the key planes)
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, unknown flags and sizes with H, W <= 0, F < 0
 * or 3 F H W >= 2^31; MODE_ERR_WORKSPACE for a missing or unaligned workspace.  F = 0 is a no-op. */
#define MODE_MV_CONF_PNG 1
#define MODE_MV_DEPTH_ONLY 2
size_t mode_multiview_handoff_workspace_bytes(int F, int H, int W);

int mode_multiview_handoff(const float* disp, const float* conf, int F, int H, int W, const float* baselines6, const float* rot_grids,
                           const float* trig, const double* xforms, int flags, float* out, void* workspace, mode_stream_t stream);

/* The gradient of the hand-off's DEPTH channels with respect to the disparities, in two launches and without a memset (every element
 * of gdisp (F, 6, H, W) is written; graph-capturable).  gout is the gradient of `out` in the forward's layout, (F, 12, H, W) or
 * (F, 6, H, W) under MODE_MV_DEPTH_ONLY; its confidence channels are not read by this entry (the entry below reads them).  With S(d, j) = -(pi / W) baseline cos(phi_l) / sin^2(d pi / W) where d != 0 and the
 * unclipped sine-rule depth lies in [0, 1000], and exactly +0 elsewhere:
 *   12        gdisp = gout S
 *   13, 14    gdisp[s] = S sum_k weight[k] gout[target[k]] over the adjoint list of source s (float32, stored order, no atomics)
 *   23 24 34  the z-buffer's winner alone: gdisp[winner(t)] = gout[t] (r1 - dir . t_xf) / r2 S unless the target is capped at 1000;
 *             every other source +0.  The winner is decoded from the forward's key.
 *   keys        device, 8-byte aligned: the forward's workspace after mode_multiview_handoff on the same disp (3 F H W keys)
 *   baselines6, trig, xforms   as the forward's
 *   adj_rowptr  device int32 (2, H W + 1): for grid 13, then 14, the range of entries of every source pixel; offsets into
 *   adj_target, adj_weight     device, n_adj entries (n_adj <= 8 H W): target pixel and bilinear weight, sorted by source, target, corner
 * Arguments are checked before any launch as the forward's are (MODE_ERR_WORKSPACE for missing or unaligned keys).  F = 0 is a no-op.
 * The CONTENTS of the device arrays cannot be checked on the host: the kernels stay inside the buffers whatever they hold (list ranges
 * are clamped to [0, n_adj], targets and decoded winners outside the plane are skipped), but a malformed list, or keys of another
 * size or another disp, give undefined gradient values, not a diagnostic. */
int mode_multiview_handoff_bwd(const float* disp, const float* gout, const void* keys, int F, int H, int W, const float* baselines6,
                               const float* trig, const double* xforms, const int32_t* adj_rowptr, const int32_t* adj_target,
                               const float* adj_weight, int n_adj, int flags, float* gdisp, mode_stream_t stream);

/* The same with the gradient of the CONFIDENCE channels beside it: the arguments of the entry above and gconf (F, 6, H, W), both
 * outputs written in the same two launches (every element; structural zeros are +0.0; the adjoint lists are walked once per source
 * for both).  gdisp has the bits of the entry above.  With q the identity the confidence channels are linear in conf:
 *   12        gconf = gout[f, 1], copied
 *   13, 14    gconf[s] = sum_k weight[k] gout[f, 2p + 1, target[k]] over the adjoint list of source s (float32, stored order), for
 *             every source: the confidence does not depend on the disparity, so sources with disp == 0 get their sum too
 *   23 24 34  gconf[winner(t)] = gout[f, 2p + 1, t], every other source +0; a winner capped at 1000 or without a slope passed its
 *             confidence on in the forward and gets this gradient all the same
 * MODE_ERR_BAD_ARG under MODE_MV_DEPTH_ONLY (no confidence channels) and under MODE_MV_CONF_PNG (the 8-bit rounding q is piecewise
 * constant: it has no gradient); otherwise the checks of the entry above. */
int mode_multiview_handoff_bwd_full(const float* disp, const float* gout, const void* keys, int F, int H, int W, const float* baselines6,
                                    const float* trig, const double* xforms, const int32_t* adj_rowptr, const int32_t* adj_target,
                                    const float* adj_weight, int n_adj, int flags, float* gdisp, float* gconf, mode_stream_t stream);

/* The hand-off for any camera rig (csrc/multiview_rig.hip): the contract of the four entries above with 6 -> P.  A frame has P pairs,
 * 1 <= P <= MODE_MV_MAX_PAIRS, of any kind in any order, described by P host records:
 *   kind      MODE_MV_IDENTITY  the sine rule alone                                  (as pair 12 above)
 *             MODE_MV_ROTATE    + the bilinear border gather on rot_grids[table]      (as pairs 13, 14)
 *             MODE_MV_VIEW      + the view transform xforms[table] with its z-buffer  (as pairs 23, 24, 34)
 *   table     the pair's index into rot_grids, 0 <= table < R, or into xforms and the key planes, 0 <= table < V; ignored for
 *             MODE_MV_IDENTITY.  The R rotate pairs name R different grids and the V view pairs V different transforms
 *   baseline  of the pair
 * disp, conf (F, P, H, W) -> out (F, 2P, H, W) with out[f, 2p] = depth, out[f, 2p + 1] = q(confidence), or (F, P, H, W) of the depths
 * under MODE_MV_DEPTH_ONLY; MODE_MV_CONF_PNG as above.  Every plane has the bits the single-map entries give for its pair.
 *   R, rot_grids  the number of rotate pairs and their grids, device (R, H, W, 2), 8-byte aligned; NULL when R == 0
 *   V, xforms     the number of view pairs and their V x (R[9] row-major, t[3]), host; NULL when V == 0
 *   trig          device, as mode_depth_view_trans; NULL when V == 0
 *   workspace     device, 8-byte aligned, >= mode_multiview_rig_handoff_workspace_bytes(F, V, H, W) = V F H W 8 bytes: key plane
 *                 (f, table) at word (f V + table) H W.  With V == 0 it may be NULL, and neither the fill nor the resolve is launched
 *                 (one launch; three otherwise, whatever F and P are).  The _bytes entry returns 0 for sizes the entries refuse
 * The gradient entries take the forward's records, trig and xforms, the key planes it left behind (NULL when V == 0) and the adjoint
 * lists of the R grids: adj_rowptr device int32 (R, H W + 1), offsets into adj_target / adj_weight of n_adj <= 4 R H W entries (NULL
 * when R == 0).  Two launches, one when V == 0; no atomics, no memset, every element of gdisp (and gconf) (F, P, H, W) written.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for P < 1 or P > MODE_MV_MAX_PAIRS, an unknown kind, R or V that is not the
 * number of pairs of that kind, a table index out of range or named twice, NULL pointers, unknown flags, H, W <= 0, F < 0 or
 * 2 P F H W >= 2^31; MODE_ERR_WORKSPACE for a missing or unaligned workspace / key planes when V > 0; _bwd_full refuses
 * MODE_MV_DEPTH_ONLY and MODE_MV_CONF_PNG as the entry above does.  F = 0 is a no-op.  What the device arrays hold cannot be checked,
 * as above. */
#define MODE_MV_MAX_PAIRS 16
#define MODE_MV_IDENTITY 0
#define MODE_MV_ROTATE 1
#define MODE_MV_VIEW 2
typedef struct mode_mv_pair {
  int32_t kind;
  int32_t table;
  float baseline;
} mode_mv_pair;

size_t mode_multiview_rig_handoff_workspace_bytes(int F, int V, int H, int W);

int mode_multiview_rig_handoff(const float* disp, const float* conf, int F, int P, int H, int W, const mode_mv_pair* pairs, int R,
                               const float* rot_grids, const float* trig, int V, const double* xforms, int flags, float* out,
                               void* workspace, mode_stream_t stream);

int mode_multiview_rig_handoff_bwd(const float* disp, const float* gout, const void* keys, int F, int P, int H, int W,
                                   const mode_mv_pair* pairs, int R, const float* trig, int V, const double* xforms,
                                   const int32_t* adj_rowptr, const int32_t* adj_target, const float* adj_weight, int n_adj, int flags,
                                   float* gdisp, mode_stream_t stream);

int mode_multiview_rig_handoff_bwd_full(const float* disp, const float* gout, const void* keys, int F, int P, int H, int W,
                                        const mode_mv_pair* pairs, int R, const float* trig, int V, const double* xforms,
                                        const int32_t* adj_rowptr, const int32_t* adj_target, const float* adj_weight, int n_adj,
                                        int flags, float* gdisp, float* gconf, mode_stream_t stream);

/* Training forward of convbn_3d (models/submodule.py:20-22) without the statistics pass: the stride-1 split-bf16 convolution kernel
 * takes the BatchNorm batch statistics of its output from the accumulators (per channel: sum(y - K), sum((y - K)^2), K = the layer's own
 * first output value) and leaves them in `stats` = the BatchNorm workspace (>= mode_bn_workspace_bytes(Co) bytes) as
 * mode_conv3d_fwd_split_stats_partials() pairs per channel + the pivots; mode_bn_train_fwd_prestats(..., nsplit = that number, ...) then
 * is mode_bn_train_fwd minus its statistics kernel (one statistics group).  Needs mode_conv3d_split_supported(Ci, Co, 1, 0) == 1. */
int mode_conv3d_fwd_split_stats_partials(void);
int mode_conv3d_fwd_split_stats(const float* x, const float* w, float* y, float* wpack, float* stats, int B, int Ci, int D, int H, int W,
                                int Co, mode_stream_t stream);
int mode_bn_train_fwd_prestats(const float* y, const float* add, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu, float* out,
                               float* save_mean, float* save_invstd, float* save_scale, float* save_shift, float* workspace, int nsplit,
                               int B, int C, long long S, mode_stream_t stream);
int mode_bn_train_fwd_prestats_amax(const float* y, const float* add, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu, float* out,
                                    float* save_mean, float* save_invstd, float* save_scale, float* save_shift, float* workspace,
                                    int nsplit, int B, int C, long long S, float* out_absmax /* as mode_bn_train_fwd_amax */,
                                    mode_stream_t stream);

/* out = a + b [+ c [+ d]] (c, d may be NULL; fixed association): the gradient of a tensor with several consumers in ONE pass.
 * No reference counterpart as code: autograd's pairwise accumulation of the gradients of cost0 / pre1
 * (models/mode_disparity.py:119-125) is what it replaces.  n elements, 16-byte aligned buffers. */
int mode_sum_n(const float* a, const float* b, const float* c, const float* d, float* out, long long n, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fusion network (models/mode_fusion.py:91-307, built as train_fusion.py:64): the layers that are neither a 3x3
 * convolution (mode_conv2d_*) nor a BatchNorm (mode_bn_*).  csrc/fusion_ops.hip; all deterministic, fp32.
 *
 * mode_maxpool2x2_fwd / _bwd: nn.MaxPool2d(2, stride=2) (mode_fusion.py:146, :161, :190) over N = B * C planes (H, W) -> (H / 2, W / 2),
 *   floor; picks like torch (scan order, a later value replaces the current one when it is greater or NaN); the backward recomputes
 *   the choice from x (no index tensor) and writes all of gx (zeros where nothing was picked).
 * mode_depth_to_space2 / mode_space_to_depth2: the rearrangement half of nn.ConvTranspose2d(Ci, Co, 2, 2) (mode_fusion.py:195, :212) --
 *   kernel 2, stride 2: no overlapping taps, so the layer is ONE 1x1 convolution with 4 Co output channels (row 4 o + 2 i + j of the
 *   weight's own (Ci, 4 Co) storage: mode_conv1x1_bwd_data on x with the weight as it lies) followed by
 *       y[b, o, 2h+i, 2w+j] = relu?(scale[o] * y4[b, 4 o + 2 i + j, h, w] + shift[o])        (scale NULL = 1, shift NULL = 0)
 *   with the bias (training) or the bias and the folded eval-mode BatchNorm (inference) as the per-channel affine.  The inverse
 *   rearranges the output gradient for mode_conv1x1_fwd (input gradient) / mode_conv1x1_bwd_weight (weight gradient).
 * mode_conv1x1_sigmoid_fwd / _bwd: nn.Conv2d(C, 1, 1, bias=True) + nn.Sigmoid (mode_fusion.py:228-229) over (B, C, S) planes, S % 4 == 0,
 *   C <= 64: s = sigmoid(bias + sum_c w[c] x[b, c, :]).  bwd: gs = dL/ds -> gx (B, C, S) written (may be NULL), gw (C) and gbias (1, may be
 *   NULL) written (accumulate = 0) or added to (accumulate = 1); workspace >= mode_conv1x1_sigmoid_bwd_workspace_bytes(B, S). */
int mode_maxpool2x2_fwd(const float* x, float* y, long long N, int H, int W, mode_stream_t stream);
int mode_maxpool2x2_bwd(const float* x, const float* gy, float* gx, long long N, int H, int W, mode_stream_t stream);
int mode_depth_to_space2(const float* y4, const float* scale, const float* shift, float* y, int B, int Co, int H, int W, int relu,
                         mode_stream_t stream);
int mode_space_to_depth2(const float* gy, float* g4, int B, int Co, int H, int W, mode_stream_t stream);
int mode_conv1x1_sigmoid_fwd(const float* x, const float* w, const float* bias, float* s, int B, int C, long long S, mode_stream_t stream);
size_t mode_conv1x1_sigmoid_bwd_workspace_bytes(int B, long long S);
int mode_conv1x1_sigmoid_bwd(const float* x, const float* w, const float* s, const float* gs, float* gx, float* gw, float* gbias,
                             int accumulate, float* workspace, int B, int C, long long S, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Metrics and losses (csrc/metrics.hip): the reductions of the reference's utils/evaluation.py (mae, max_ae, rmse, absrel, sqrel,
 * silog, pixel_error_pct, D1, delta_acc, threshold_acc: :4-55) and the SILog training loss of the fusion stage (train_fusion.py:82-87,
 * applied at :99-111).  All deterministic (two launches, a fixed summation order that depends on n only, no atomics).
 *
 * mode_masked_metrics: ONE pass over pred, gt (fp32, n elements) and mask (n bytes, nonzero = selected; NULL = every element) that
 *   writes out[MODE_METRICS_COUNT] (fp64, device) with the statistics below over the selected elements -- the reference's functions on
 *   pred[mask], gt[mask], without the compaction.  Per-element terms are formed in fp32 as torch forms them: d = p - g, |d|, d * d,
 *   |d| / g, (d * d) / (g * g), p / g and g / p as IEEE fp32 operations, thresholds rounded to fp32 (torch casts a Python scalar to
 *   the tensor's dtype), t_pct * g as an fp32 product; l = log p - log g in fp64.  Sums accumulate in fp64.
 *     out[MODE_METRICS_N]          selected elements              (numel)
 *     out[MODE_METRICS_N_GT]       ... with gt > 0                (absrel, sqrel)
 *     out[MODE_METRICS_N_BOTH]     ... with gt > 0 and pred > 0   (silog)
 *     out[MODE_METRICS_SUM_ABS]    sum |d|                         out[MODE_METRICS_SUM_SQ]      sum d * d
 *     out[MODE_METRICS_SUM_ABSREL] sum |d| / g over gt > 0         out[MODE_METRICS_SUM_SQREL]   sum d*d / (g*g) over gt > 0
 *     out[MODE_METRICS_SUM_LOG]    sum l over gt, pred > 0         out[MODE_METRICS_SUM_LOG2]    sum l * l over gt, pred > 0
 *     out[MODE_METRICS_MAX_ABS]    max |d|, NaN if any |d| is NaN (torch.max); 0 for no element
 *     out[MODE_METRICS_PX + k]     count of |d| >= px[k]                                   (pixel_error_pct), k < n_px
 *     out[MODE_METRICS_D1 + k]     count of |d| >= d1_px[k] and |d| >= d1_pct[k] * g      (D1), k < n_d1
 *     out[MODE_METRICS_RATIO + k]  count of max(p / g, g / p) < ratio[k], NaN-propagating  (delta_acc, threshold_acc), k < n_ratio
 *   (NaN fails every comparison and still counts in N.)  `params` lives in host memory and is read during the call.
 *   workspace: device, 8-byte aligned, workspace_bytes >= mode_masked_metrics_workspace_bytes(n).
 * mode_silog_loss_fwd: the same pass restricted to l (mask, gt > 0, pred > 0): stats[MODE_METRICS_COUNT] (fp64, device; the l entries
 *   and N_BOTH filled, the others 0) and loss[0] = sum l^2 / N_BOTH - lamda (sum l / N_BOTH)^2 as a device fp32 scalar (NaN when
 *   N_BOTH = 0, as torch's mean of nothing).  No host synchronisation: capturable into a graph.  Workspace as mode_masked_metrics.
 * mode_silog_loss_bwd: gpred (n) = gloss[0] * (2 / N_BOTH) (l - lamda sum l / N_BOTH) / p on the selected elements, exactly 0 elsewhere
 *   (all zeros when N_BOTH = 0); `stats` as written by mode_silog_loss_fwd for the same inputs, gloss a device fp32 scalar.
 * pred, gt and gpred may be NULL when n = 0 (an empty tensor).  Bad arguments (NULL pointers, n < 0, more than MODE_METRICS_MAX_THRESHOLDS of a kind) return MODE_ERR_BAD_ARG, a missing or small
 * workspace MODE_ERR_WORKSPACE, before any launch. */
#define MODE_METRICS_MAX_THRESHOLDS 4
#define MODE_METRICS_N 0
#define MODE_METRICS_N_GT 1
#define MODE_METRICS_N_BOTH 2
#define MODE_METRICS_SUM_ABS 3
#define MODE_METRICS_SUM_SQ 4
#define MODE_METRICS_SUM_ABSREL 5
#define MODE_METRICS_SUM_SQREL 6
#define MODE_METRICS_SUM_LOG 7
#define MODE_METRICS_SUM_LOG2 8
#define MODE_METRICS_MAX_ABS 9
#define MODE_METRICS_PX 10
#define MODE_METRICS_D1 (MODE_METRICS_PX + MODE_METRICS_MAX_THRESHOLDS)
#define MODE_METRICS_RATIO (MODE_METRICS_D1 + MODE_METRICS_MAX_THRESHOLDS)
#define MODE_METRICS_COUNT (MODE_METRICS_RATIO + MODE_METRICS_MAX_THRESHOLDS)
typedef struct mode_metrics_params {
  int n_px; /* pixel_error_pct thresholds used */
  float px[MODE_METRICS_MAX_THRESHOLDS];
  int n_d1; /* D1 (th_pixel, th_pct) pairs used */
  float d1_px[MODE_METRICS_MAX_THRESHOLDS];
  float d1_pct[MODE_METRICS_MAX_THRESHOLDS];
  int n_ratio; /* ratio bounds used (delta_acc: 1.25^exp, threshold_acc: 1 + err_pct) */
  float ratio[MODE_METRICS_MAX_THRESHOLDS];
} mode_metrics_params;
size_t mode_masked_metrics_workspace_bytes(long long n);
int mode_masked_metrics(const float* pred, const float* gt, const uint8_t* mask, long long n, const mode_metrics_params* params,
                        void* workspace, size_t workspace_bytes, double* out, mode_stream_t stream);
int mode_silog_loss_fwd(const float* pred, const float* gt, const uint8_t* mask, long long n, float lamda, void* workspace,
                        size_t workspace_bytes, double* stats, float* loss, mode_stream_t stream);
int mode_silog_loss_bwd(const float* pred, const float* gt, const uint8_t* mask, long long n, float lamda, const double* stats,
                        const float* gloss, float* gpred, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring in the equirectangular (ERP) domain (csrc/erp_metrics.hip): what the reference's test_fusion.py does per batch between
 * the fusion network and its metric table (:82, :86-100).
 *
 * mode_erp_depth_metrics (test_fusion.py:86-100): for each of `frames` Cassini maps pred, gt (frames, H, W), H == 2 W, ONE pass that
 *   resamples both to the ERP panorama (W rows, H columns) through `grid` -- (W, H, 2) normalised (x, y) sample points, the table of
 *   cassini2Equirec; bilinear, border padding, align_corners = true: the arithmetic of mode_grid_sample_border --, selects the ERP
 *   pixels with gt_erp <= maxdepth (plain fp32 comparison: NaN is not selected) and reduces the statistics of mode_masked_metrics over
 *   them, per frame: out (frames, MODE_METRICS_COUNT) fp64, device.  pred_erp / gt_erp, each (frames, W, H) or NULL, receive the
 *   resampled maps.  Two launches, no atomics, no host synchronisation (capturable into a graph).  Row f depends on frame f alone and
 *   has the bits of mode_masked_metrics on that frame's ERP maps (from mode_grid_sample_border) and mask: within a frame, ERP pixel
 *   quads are dealt to threads exactly as that entry deals the elements of a flat range of H * W.
 *   workspace: device, 8-byte aligned, workspace_bytes >= mode_erp_depth_metrics_workspace_bytes(frames, H, W)
 *   (= frames * mode_masked_metrics_workspace_bytes(H * W)).  grid: 8-byte aligned.  frames == 0 returns MODE_OK without a launch.
 * mode_bicubic_up2 (test_fusion.py:82, --resize): (N, C, H, W) -> (N, C, 2H, 2W) as F.interpolate(scale_factor=[2, 2], mode='bicubic',
 *   align_corners=True): source coordinate o * (in - 1) / (out - 1), cubic convolution with A = -0.75, border-clamped taps, 16 fp32
 *   products per output.  The four corners of a plane are copied exactly.
 * Bad arguments return MODE_ERR_BAD_ARG, a missing or small workspace MODE_ERR_WORKSPACE, before any launch. */
size_t mode_erp_depth_metrics_workspace_bytes(int frames, int H, int W);
int mode_erp_depth_metrics(const float* pred, const float* gt, const float* grid, int frames, int H, int W, float maxdepth,
                           const mode_metrics_params* params, void* workspace, size_t workspace_bytes, double* out, float* pred_erp,
                           float* gt_erp, mode_stream_t stream);
int mode_bicubic_up2(const float* src, float* dst, int N, int C, int H, int W, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 8-bit ingest of whole frames (csrc/ingest.hip): what the reference's loaders do on the host between the decoded PNGs and the two
 * networks.  frames_u8 is the one buffer of this header that is not fp32: (F, 12, H, W, 3) bytes, the 12 panoramas of a frame in
 * sorted file order, each as np.asarray(PIL image) lays it out; 4-byte aligned.  lut is the device table (256, 3) fp32 with
 * lut[v][c] = the bits of ((v / 255) - mean[c]) / std[c] as the host transform rounds it (dataloader/preprocess.py:8, 64-69:
 * ToTensor + Normalize with the ImageNet statistics); the kernels only look values up.
 *
 * mode_frames_u8_ingest (deep360_loader.py:108-109, 161-163): norm = the table lookup on every byte, planar (3, H, W) fp32 out:
 *     left[6 f + p] = norm(frames[f, 2 p]), right[6 f + p] = norm(frames[f, 2 p + 1])      (6 F, 3, H, W) each
 *     rgb[f] = the 12 planes of panoramas 0, 1, 10, 11 of frame f                           (F, 12, H, W), or NULL = not wanted
 *   H W % 4 == 0; outputs 16-byte aligned.  One launch: three dwords (four pixels) in and one 16-byte store per plane per thread.
 * mode_rgb_half_pil (deep360_loader.py:151-153, 161-163): panoramas 0, 1, 10, 11 of every frame halved exactly as Pillow's
 *   Image.resize((W / 2, H / 2)) halves an RGB image (Resample.c, bicubic a = -0.5, support 4, 8 bits per channel: the horizontal
 *   pass, its result stored in 8 bits, the vertical pass; per pass clip((2^21 + sum_j px_j kk_j) >> 22, 0, 255) in 32-bit integers),
 *   then norm: rgb_half (F, 12, H / 2, W / 2) fp32; half_u8 (F, 4, H / 2, W / 2, 3) bytes receives the 8-bit result, or NULL.
 *   tab_w (W / 2, 10), tab_h (H / 2, 10) int32, device: per output index the first input index, the number of taps (<= 8) and 8
 *   fixed-point coefficients kk = int(k 2^22 +/- 0.5), built on the host in double (dataloader.preprocess.pil_half_table).  H and W even.
 *   One launch: a workgroup owns 16 x 32 output pixels and keeps the horizontal pass of the 38 input rows under them in LDS.
 * mode_decimate2 (deep360_loader.py:147-150): out[n, y, x] = in[n, 2 y, 2 x] over `planes` fp32 planes (H, W) -> (ceil(H / 2), ceil(W / 2)),
 *   the [::2, ::2] of the loader on the planes of mode_multiview_handoff.
 * mode_decimate2_bwd: its adjoint, gin[n, y, x] = gout[n, y / 2, x / 2] where y and x are both even and +0.0 elsewhere; every element of
 *   gin (planes, H, W) is written, in one launch with 16-byte stores (gin 16-byte aligned; single stores otherwise).  Sizes as the forward.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, misaligned buffers, H, W <= 0, F or planes < 0, sizes
 * the entry does not take and element counts (36 F H W, planes H W) >= 2^31.  F = 0 / planes = 0 is a no-op. */
int mode_frames_u8_ingest(const uint8_t* frames_u8, const float* lut, int F, int H, int W, float* left, float* right, float* rgb,
                          mode_stream_t stream);
int mode_rgb_half_pil(const uint8_t* frames_u8, const int32_t* tab_w, const int32_t* tab_h, const float* lut, int F, int H, int W,
                      float* rgb_half, uint8_t* half_u8, mode_stream_t stream);
int mode_decimate2(const float* in, float* out, long long planes, int H, int W, mode_stream_t stream);
int mode_decimate2_bwd(const float* gout, float* gin, long long planes, int H, int W, mode_stream_t stream);

/* Colour augmentation on the 8-bit ingest (csrc/augment.hip): the reference's inception_color_preproccess
 * (dataloader/preprocess.py:33-46: ToTensor, ColorJitter(0.4, 0.4, 0.4), Lighting(0.1, eigval, eigvec), Normalize; Lighting is
 * preprocess.py:78-95) on N images, fused with the planar split.  The random draws are the host's; the kernels read them from two
 * device tables.  Per image, in fp32, every operation rounded once to nearest, in this order, nothing contracted:
 *     x = (float)v / 255.0f                                           (IEEE division)
 *     grey(x) = (0.2989f * r + 0.587f * g) + 0.114f * b
 *     blend(a, b, k) = clamp(rho_k * a + sigma_k * b, 0, 1)           rho_k the factor, sigma_k = (float)(1.0 - factor) formed by
 *                                                                     the host in double: the kernel never computes 1 - rho
 *     up to three operations in the image's own order:
 *       brightness  x = blend(x, 0, b)
 *       contrast    x = blend(x, m, c), m = the mean of grey(x) over the H W pixels as x stands when the step is reached
 *       saturation  x = blend(x, grey(x), s)                          per pixel
 *     x[c] += shift[c]                                                (Lighting: no clamp)
 *     (x[c] - mean[c]) / std[c]                                       (fp32 ImageNet statistics, IEEE division)
 *   m: the fp32 grey values are summed in fp64 in a fixed order (a thread walks its quads in ascending order, a fixed butterfly over
 *   the lanes, the waves in index order, one partial per block; the partials folded in index order), divided by H W and rounded once
 *   to fp32.  No atomics; the number of partials depends on H W alone: the same images and tables give the same bits on any
 *   stream and any device.
 * mode_images_u8_augment:
 *   images_u8 (N, H, W, 3) bytes, each image as np.asarray(PIL RGB image) lays it out; 4-byte aligned.
 *   ops (N, 3) int32, device: the image's operations in order -- 0 brightness, 1 contrast, 2 saturation, anything else: no operation.
 *     A code only selects a branch; a row should name an operation at most once (a second contrast step would blend with the mean
 *     of the first).
 *   coef (N, 9) fp32, device: rho_b, sigma_b, rho_c, sigma_c, rho_s, sigma_s, shift_r, shift_g, shift_b (indexed by operation, not by
 *     position in the order).
 *   dst (N, ndst) int32, device, or NULL; ndst = 1 or 2: image n is written to out[dst[n][j]] for every j; NULL means one slot,
 *     dst[n] = n (whatever ndst says, which must still be 1 or 2).  A slot outside [0, slots) is skipped (-1: "no second copy"; an image with no valid slot
 *     is not written).  Two images with the same slot: undefined which one stays.  ndst = 2 is what lets one call write the left /
 *     right stacks of a frame AND the second copy of the four panoramas the fusion stage takes.
 *   out (slots, 3, H, W) fp32, 16-byte aligned; slots that no image names keep their content.
 *   means (N,) fp32 or NULL: the contrast mean m used for image n, 0 for an image without a contrast step.
 *   workspace: device, 8-byte aligned, workspace_bytes >= mode_images_u8_augment_workspace_bytes(N, H, W); it needs no initialisation.
 *   Two launches: the grey sums (of the images that have a contrast step, after the operations that precede it), then the whole chain.
 *   One thread handles four pixels: three dwords in, one 16-byte store per colour plane out.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, misaligned buffers, H, W <= 0, N or slots < 0,
 * ndst not 1 or 2, H W % 4 != 0, element counts (3 N H W, 3 slots H W) >= 2^31 and a workspace that is too small.  N = 0 is a no-op. */
size_t mode_images_u8_augment_workspace_bytes(int N, int H, int W);
int mode_images_u8_augment(const uint8_t* images_u8, const int32_t* ops, const float* coef, const int32_t* dst, int ndst, int N, int H,
                           int W, int slots, float* out, float* means, void* workspace, size_t workspace_bytes, mode_stream_t stream);

/* Stereo pairs at any working size (csrc/resize.hip): what the reference's Deep360DatasetDisparity does on the host when a
 * pair is stored at another width than the working one (dataloader/deep360_loader.py:92-106), on the decoded data.
 *
 * mode_images_u8_resize_pil: N images (N, Hs, Ws, 3) bytes, each as np.asarray(PIL RGB image) lays it out (no alignment asked for:
 *   bytes are read one at a time), resized to (H, W) exactly as Pillow's Image.resize((W, H)) resizes an RGB image -- Resample.c,
 *   the default bicubic filter (a = -0.5), 8 bits per channel: the horizontal pass, its result stored in 8 bits, the vertical pass; per
 *   pass clip((2^21 + sum_j px_j kk_j) >> 22, 0, 255) in 32-bit integers; a pass whose size does not change is skipped (with both
 *   skipped the entry copies).
 *   MODE_RESIZE_MAX_SCALE: along either axis the sizes may differ by a factor of 4 at most, in either direction (Hs <= 4 H, H <= 4 Hs,
 *   likewise the widths; any ratio inside that, different ones per axis).  Anything beyond returns MODE_ERR_UNSUPPORTED before a
 *   pointer is looked at.
 *   tab_w (W, 2 + ksize_w), tab_h (H, 2 + ksize_h) int32, device: per output index the first source index, the number of taps
 *     (<= ksize) and ksize fixed-point coefficients kk = int(k 2^22 +/- 0.5), built on the host in double
 *     (dataloader.preprocess.pil_resize_table); 1 <= ksize <= 17.  The table of a skipped pass is not read and may be NULL.
 *   lut: the (256, 3) table of the other ingest entries; needed with `out`.
 *   windows (ceil(N / per_window), 2) int32, device, or NULL: (top, left) of the (h_win, w_win) window of the resized (H, W) image that
 *     is computed and stored for images n with n / per_window = the row (per_window = 2: both images of a pair share a window).
 *     NULL: (0, 0) for every image; the whole image is h_win = H, w_win = W.  A window is moved inside the image where the table would
 *     put it outside.  Nothing outside the window is computed, and the full resized image is not stored anywhere.
 *   out_u8 (N, h_win, w_win, 3) bytes and / or out (N, 3, h_win, w_win) fp32 = the table lookup of those bytes; either may be NULL, not
 *     both.  split = 1 (N a multiple of per_window): image n goes to slot (n % per_window) * (N / per_window) + n / per_window of
 *     both outputs -- the left images of N / 2 pairs first, then the right ones; split = 0: slot n.
 *   workspace: device, mode_images_u8_resize_pil_workspace_bytes(...) bytes -- the 8-bit result of the horizontal pass,
 *     (N, Hs, w_win, 3), of which only the rows the window's vertical taps reach are written and read; 0 bytes (workspace may be NULL)
 *     when at most one pass runs.  It needs no initialisation.
 *   One launch per pass that runs; a thread per output pixel of the pass and a plain loop over the taps.
 * mode_disp_resize_nearest: out[n, y, x] = disp[n, rows[top + y], cols[left + x]] * ratio for N fp32 maps (N, Hs, Ws) -> (N, h_win, w_win):
 *   cv2.resize(..., (W, H), INTER_NEAREST) * (W / Ws) and the same window.  rows (H,), cols (W,) int32, device: the source index
 *   min(floor(i * (src / dst)), src - 1) formed in double on the host (clamped to the map here); ratio: one fp32 multiply, NaN stays
 *   NaN.  windows (N, 2) or NULL as above with one row per map.  Any sizes.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, misaligned tables, non-positive sizes, N < 0, a window
 * that does not fit into (H, W), ksize outside 1 .. 17, per_window < 1 and element counts (3 N Hs max(Ws, W), 3 N H W; N Hs Ws, N H W
 * for the maps) >= 2^31; MODE_ERR_WORKSPACE for a missing or small workspace.  N = 0 is a no-op. */
#define MODE_RESIZE_MAX_SCALE 4
size_t mode_images_u8_resize_pil_workspace_bytes(int N, int Hs, int Ws, int H, int W, int h_win, int w_win);
int mode_images_u8_resize_pil(const uint8_t* images_u8, const int32_t* tab_w, int ksize_w, const int32_t* tab_h, int ksize_h,
                              const float* lut, const int32_t* windows, int per_window, int split, int N, int Hs, int Ws, int H, int W,
                              int h_win, int w_win, uint8_t* out_u8, float* out, void* workspace, size_t workspace_bytes,
                              mode_stream_t stream);
int mode_disp_resize_nearest(const float* disp, const int32_t* rows, const int32_t* cols, const int32_t* windows, int N, int Hs, int Ws,
                             int H, int W, int h_win, int w_win, float ratio, float* out, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 3D60 ingest (csrc/erp_ingest.hip): what the reference's Dataset3D60Disparity.__getitem__ (dataloader/dataset3D60Loader.py:123-248)
 * does on the host per sample between the decoded equirectangular (ERP) files and ModeDisparity, for a batch of N pairs.
 *
 * The re-projection of both entries is F.grid_sample(bilinear, border, align_corners = true) with the BITS of torch's CPU kernel
 * (the RGB result is truncated to bytes; a sum that is only close is off by one on saturated regions).  Per output pixel, in fp32,
 * every operation rounded to nearest, for a source of (Hs, Ws) and a grid point (gx, gy):
 *     x  = min(max((gx + 1) * ((Ws - 1) / 2), 0), Ws - 1)             likewise y with Hs
 *     x0 = floor(x); ex = x - x0; wx = 1 - ex                         likewise y0, ey, wy
 *     nw = wx * wy; ne = ex * wy; sw = wx * ey; se = ex * ey
 *     v  = fma(p_se, se, fma(p_sw, sw, fma(p_ne, ne, p_nw * nw)))     corners outside the image are not read and count as 0
 *
 * mode_erp_pairs_u8_cassini (dataset3D60Loader.py:177-180, 192-193, 202-205, 232-236):
 *   pairs_u8 (N, 2, He, We, 3) bytes: left and right ERP panorama of N samples as np.asarray(PIL RGB image) lays them out.
 *   grid (G, H, W, 2) fp32, G = 1 or N: the sample points of utils.geometry.erp2rect_cassini for the pair's rotation, built on the
 *     host (utils.geometry.erp2rect_grid); 16-byte aligned.  G = 1: one grid serves every sample.
 *   lut (256, 3): the table of mode_frames_u8_ingest.
 *   left, right (N, 3, H, W) fp32 = lut[trunc(bilinear)]: erp2rect_cassini(...).astype(np.uint8), then the stage-1 transform.
 *   left_flip, right_flip (N, 3, H, W) or both NULL: the mirrored twin (:193):
 *     left_flip[.., x] = right[.., W-1-x], right_flip[.., x] = left[.., W-1-x].
 *   cassini_u8 (N, 2, H, W, 3) or NULL: the 8-bit Cassini images themselves; 4-byte aligned.
 * mode_erp_depth_disp (dataset3D60Loader.py:182-185, 192-196, 209-210, 258-270):
 *   depth_erp (N, He, We) fp32 -> disparity ground truth disp (N, 1, H, W):
 *     d = bilinear (same arithmetic, fp32 result kept); d > maxdepth -> 0; invalid (d <= 0) -> NaN; else
 *     disp = W * (asin(clip((d*s_j + b) / sqrt(d*d + b*b - 2*d*b*c_j), -1, 1)) - phi_j) / pi, negative -> 0,
 *   in numpy's order of operations and numpy 2's types: the products of two arrays (d*s_j, d*d) in fp32, everything from the first
 *   scalar on in fp64 (the reference's masked array is promoted there), one rounding to fp32 on the store.  `baseline` is widened to
 *   fp64 as it is: 0.26f lies 3.7e-8 (relative) below the reference's double 0.26, which moves a disparity by at most 2e-6 px.
 *   cols (3, W) fp32, 16-byte aligned: phi_j, s_j = sin(phi_j), c_j = cos(phi_j + pi/2) as numpy rounds them, host-built.
 *   mirror != 0 writes column W-1-x of the re-projected depth to column x BEFORE the sine rule (the flip twin, fed the right view's
 *     depth).  depth_cassini (N, H, W) or NULL: the re-projected, thresholded depth.
 * One launch each: a thread owns four consecutive pixels of a Cassini row (one 16-byte store per fp32 plane) and forms the weights
 * once for both images, all channels and -- with G = 1 -- all samples it walks.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, misaligned grid / cols / outputs (16 bytes),
 * G not in {1, N}, He or We < 2, W % 4 != 0, N < 0 and element counts (6 N He We, 6 N H W, 2 G H W) >= 2^31.  N = 0 is a no-op. */
int mode_erp_pairs_u8_cassini(const uint8_t* pairs_u8, const float* grid, const float* lut, int N, int He, int We, int H, int W, int G,
                              float* left, float* right, float* left_flip, float* right_flip, uint8_t* cassini_u8, mode_stream_t stream);
int mode_erp_depth_disp(const float* depth_erp, const float* grid, const float* cols, int N, int He, int We, int H, int W, int G,
                        float baseline, float maxdepth, int mirror, float* disp, float* depth_cassini, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Spatial pyramid pooling of the PSMNet extractor, ModeDisparity(conv='Regular') (models/submodule.py:228-268):
 * the poolings, the bilinear upsamplings and the concatenation around the four branch convolutions.  csrc/spp.hip; NCHW fp32, no
 * atomics, fixed summation order (bit-repeatable), nothing allocated.  Level l = 0..3 pools k = 8 << l; its planes have
 * floor(H / k) x floor(W / k) pixels (torch's floor semantics: trailing rows and columns belong to no block).
 *
 * mode_spp_pool_fwd: x (planes, H, W) -> the four nn.AvgPool2d((k, k), stride=(k, k)) results y8, y16, y32, y64 in one pass that reads
 *   x once (a workgroup reduces a 64 x 64 region level by level; block j of level 2k is blocks 2j, 2j+1 of level k).
 * mode_spp_pool_bwd: gskip (N, Cs, H, W), written once, = channels c0 .. c0 + Cs of gcat (N, C, H, W), read where they lie (gcat NULL:
 *   no such term), + for every level g_k[n, c, h / k, w / k] / k^2 inside the level's crop; g_k (N, Cs, H / k, W / k).
 * mode_spp_concat_fwd: out (N, Cr + Cs + 4 Cb, H, W) = cat(raw (N, Cr, H, W), skip (N, Cs, H, W), up(b8), up(b16), up(b32), up(b64)), the
 *   reference's order; b_k (N, Cb, H / k, W / k); up = F.interpolate(size=(H, W), mode='bilinear', align_corners=True) with aten's fp32
 *   arithmetic: scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1 (a
 *   1-pixel source axis broadcasts).  One launch; every output element written exactly once.
 * mode_spp_concat_bwd: from gcat (N, Cr + Cs + 4 Cb, H, W): graw (N, Cr, H, W), a contiguous copy, and the four branch gradients
 *   gb_k (N, Cb, H / k, W / k), the adjoint of the upsampling in gather form: every low-resolution pixel sums the pixels whose taps
 *   touch it (support and weights from the forward's index arithmetic), one wave or one workgroup per pixel with a fixed tree.  The
 *   skip channels of gcat are left to mode_spp_pool_bwd.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, non-positive sizes and a channel range outside gcat;
 * MODE_ERR_UNSUPPORTED for H or W < 64 (the k = 64 level would be empty; the reference's pooling fails there too), planes of 2^30
 * elements or more, more than 65535 planes (N x channels) in one call or 2^31 workgroups.  N = 0 / planes = 0 is a no-op. */
int mode_spp_pool_fwd(const float* x, float* y8, float* y16, float* y32, float* y64, long long planes, int H, int W, mode_stream_t stream);
int mode_spp_pool_bwd(const float* gcat, int C, int c0, const float* g8, const float* g16, const float* g32, const float* g64, float* gskip,
                      int N, int Cs, int H, int W, mode_stream_t stream);
int mode_spp_concat_fwd(const float* raw, const float* skip, const float* b8, const float* b16, const float* b32, const float* b64, float* out,
                        int N, int Cr, int Cs, int Cb, int H, int W, mode_stream_t stream);
int mode_spp_concat_bwd(const float* gcat, float* graw, float* gb8, float* gb16, float* gb32, float* gb64, int N, int Cr, int Cs, int Cb,
                        int H, int W, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The optimizer of the training step (train_disparity.py:293: optim.Adam(params, lr, betas=(0.9, 0.999))).  csrc/optim.hip:
 * one update rule for all parameter tensors and all parameter groups in THREE launches, none of which depends on a host value
 * that changes from step to step (capturable), with a guard against non-finite gradients and the global gradient norm as a by-product.
 * No atomics, a summation order that depends on n alone: bit-repeatable on any stream.
 *
 * Data (all device memory of the caller):
 *   grad, exp_avg, exp_avg_sq: three flat fp32 buffers of n elements in ONE layout: segment after segment, no padding.
 *   segments[n_seg] (mode_adam_segment): one per parameter tensor: its address, its first element in the flat layout, its size and
 *     its group.  chunks[n_chunks] (mode_adam_chunk): at most MODE_ADAM_CHUNK elements each, every chunk inside ONE segment (off is
 *     the chunk's first element in the flat layout), together covering every element exactly once; built once by the caller.
 *   block: mode_adam_block_bytes(n_groups) bytes, 8-byte aligned, zeroed by the caller before the first step:
 *     doubles [0, MODE_ADAM_STATE_DOUBLES): the state (MODE_ADAM_STEP .. below), written by mode_adam_prepare only;
 *     doubles [8 + 8 g, 8 + 8 g + 8), g < n_groups: the group's hyper-parameters lr, beta1, beta2, eps, weight_decay, max_grad_norm
 *       (<= 0: no clipping) and two unused, written by the caller (and only by the caller);
 *     then 8 + 8 n_groups floats that mode_adam_prepare derives for mode_adam_update (word 0: the decision, 1 = skip).
 * mode_adam_prepare: sum of squares of grad in fp64 (the square of an fp32 value is exact there) and the count of non-finite
 *   elements, in the scheme of mode_masked_metrics (two launches).  The second launch decides: with skip_nonfinite != 0 and a non-finite
 *   element the step is SKIPPED (MODE_ADAM_SKIPPED + 1, MODE_ADAM_STEP unchanged); otherwise MODE_ADAM_STEP + 1 and per group
 *   step_size = lr / (1 - beta1^step), sqrt(1 - beta2^step) and clip = min(1, max_grad_norm / (norm + 1e-6)), formed in fp64 and rounded
 *   to fp32 (torch.optim.Adam's single-tensor path; torch.nn.utils.clip_grad_norm_).  MODE_ADAM_GRAD_NORM, MODE_ADAM_FOUND_INF (0 / 1)
 *   and MODE_ADAM_NONFINITE (the count) are written by every call.  workspace: 8-byte aligned, >= mode_adam_workspace_bytes(n).
 * mode_adam_update (one launch): nothing at all when the decision is "skip"; otherwise per element, in fp32, unfused, in torch's order
 *     g = grad * clip;  g = g + weight_decay * p (weight_decay != 0);  m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;
 *     p = p - step_size * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps))
 *   grad itself is left as it was.  16-byte accesses wherever the chunk's addresses in all four buffers share their alignment.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, n <= 0, n_seg / n_chunks / n_groups <= 0 and a
 * misaligned block; MODE_ERR_WORKSPACE for a missing, misaligned or small workspace.  The tables live in device memory and are trusted. */
#define MODE_ADAM_CHUNK 2048
#define MODE_ADAM_STATE_DOUBLES 8
#define MODE_ADAM_STEP 0
#define MODE_ADAM_SKIPPED 1
#define MODE_ADAM_GRAD_NORM 2
#define MODE_ADAM_FOUND_INF 3
#define MODE_ADAM_NONFINITE 4
#define MODE_ADAM_GROUP_DOUBLES 8
typedef struct mode_adam_segment {
  float* param;    /* the parameter tensor (contiguous fp32) */
  long long first; /* its first element in the flat layout */
  long long numel;
  int group;
  int unused;
} mode_adam_segment;
typedef struct mode_adam_chunk {
  long long off; /* first element in the flat layout */
  int seg;
  int count; /* 1 .. MODE_ADAM_CHUNK */
} mode_adam_chunk;
size_t mode_adam_workspace_bytes(long long n);
size_t mode_adam_block_bytes(int n_groups);
int mode_adam_prepare(const float* grad, long long n, void* workspace, size_t workspace_bytes, void* block, int n_groups,
                      int skip_nonfinite, mode_stream_t stream);
int mode_adam_update(const mode_adam_segment* segments, int n_seg, const mode_adam_chunk* chunks, int n_chunks, const float* grad,
                     float* exp_avg, float* exp_avg_sq, void* block, int n_groups, mode_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Self-supervised stereo loss on rectified Cassini pairs (csrc/photometric.hip; the reference has no counterpart: its
 * predict.py "for real scene" only loads a checkpoint).  Additive: the ABI version stays as it is.
 *
 * left, right (B, 3, H, W) fp32 as the model takes them; disp (K, B, H, W) fp32, 1 <= K <= MODE_PHOTOMETRIC_MAX_MAPS.  With
 * L = left * std + mean and R likewise, per map k:
 *   warp      x = w - d(h, w); a pixel is valid iff d is finite and 0 <= x <= W - 1; x0 = min(floor(x), W - 2), t = x - x0,
 *             Rh = (1 - t) R[h, x0] + t R[h, x0 + 1], and Rh = 0 without a gradient at invalid pixels.
 *   windows   one per (h, w) with 1 <= w <= W - 2: the 3x3 neighbourhood, rows modulo H (the long axis of a Cassini image is periodic;
 *             W runs from pole to pole and does not wrap); valid iff all nine pixels are.
 *   ssim      per channel on the window's centred, biased moments: (2 mx my + c1)(2 cxy + c2) / ((mx^2 + my^2 + c1)(vx + vy + c2)).
 *   photo_k   = sum over valid windows of mean_c[alpha (1 - ssim_c) / 2 + (1 - alpha) |L_c - Rh_c|(centre)] / max(N_valid_k, 1).
 *   smooth_k  = mean over w <= W - 2 of |dn(h, w+1) - dn(h, w)| exp(-beta mean_c |L_c(h, w+1) - L_c(h, w)|) + the mean over all pixels
 *             of the same along h (h + 1 modulo H), dn = d / W, on every pixel, valid or not.
 *   loss      = sum_k weights[k] (photo_k + lam smooth_k).  lam == 0 leaves the smoothness term out altogether, in the loss and in the
 *             gradient (a NaN disparity then costs its pixel and nothing else).
 * mode_photometric_loss_fwd: stats (K x MODE_PHOTOMETRIC_STATS fp64, device): N_valid, the sum of the windows' photometric terms and
 *   the two smoothness sums; loss: a device fp32 scalar.  Per-pixel arithmetic in fp32, accumulation in fp64 in the fixed-order scheme
 *   of mode_masked_metrics (two launches, no atomics: the same inputs give the same bits on any stream).  No host synchronisation.
 *   workspace: device, 8-byte aligned, workspace_bytes >= mode_photometric_loss_workspace_bytes(K, B, H, W) (0 for sizes the entries refuse).
 * mode_photometric_loss_bwd: gdisp (K, B, H, W) = gloss[0] * d loss / d disp, every element written once by a gather (a pixel collects
 *   the up to nine windows that contain it and its smoothness neighbours; no scatter, no atomics); N_valid is a constant; sign(0) = 0
 *   for both absolute values; invalid pixels get the smoothness gradient only.  `stats` as written by the forward for the same inputs.
 * Arguments are checked before any launch: MODE_ERR_BAD_ARG for NULL pointers, K outside 1..4, B < 1, H < 3 or W < 3;
 * MODE_ERR_UNSUPPORTED when 3 B H W >= 2^31 (offsets inside an image tensor and the workgroup index are 32-bit) or W >= 2^24 (w as an
 * exact float); MODE_ERR_WORKSPACE for a missing, misaligned or small workspace. */
#define MODE_PHOTOMETRIC_MAX_MAPS 4
#define MODE_PHOTOMETRIC_STATS 4
#define MODE_PHOTOMETRIC_N_VALID 0
#define MODE_PHOTOMETRIC_SUM_PE 1
#define MODE_PHOTOMETRIC_SUM_SMOOTH_X 2
#define MODE_PHOTOMETRIC_SUM_SMOOTH_Y 3
typedef struct mode_photometric_params {
  float alpha, lam, beta, c1, c2;
  float mean[3], std[3];                    /* the normalisation the images carry (per channel) */
  float weights[MODE_PHOTOMETRIC_MAX_MAPS]; /* wgt[k]; entries at and beyond K are ignored */
} mode_photometric_params;
size_t mode_photometric_loss_workspace_bytes(int K, int B, int H, int W);
int mode_photometric_loss_fwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                              const mode_photometric_params* params, void* workspace, size_t workspace_bytes, double* stats, float* loss,
                              mode_stream_t stream);
int mode_photometric_loss_bwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                              const mode_photometric_params* params, const double* stats, const float* gloss, float* gdisp,
                              mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_H_ */
