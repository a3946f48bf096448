/* mode_hip_selfsup.h -- the second public header of libmode_hip.so: bidirectional self-supervised stereo loss.
 *
 * include/mode_hip.h is frozen at ABI 31 by its tests (the count of its prototypes, launching entries, constants and records is
 * pinned); entries added after it are declared here.  mode_hip/_header.py reads this file on its own, exactly as it reads the first
 * header, so the constants below are integer literals (csrc/ holds static_asserts that tie them to the first header's).
 * The conventions are the first header's: plain C, device pointers unless stated, the stream is the last parameter and is named
 * `stream`, every argument is checked before any launch, no state is kept between calls, MODE_OK / MODE_ERR_* are the return codes and
 * mode_last_error() has the text.  This header has a version of its own, MODE_SELFSUP_VERSION / mode_selfsup_version().
 *
 * All maps are fp32.  disp_l, disp_r (K, B, H, W), 1 <= K <= 4.  H is Cassini's periodic axis; W runs pole to pole and does not wrap.
 * csrc/cost_volume.hip fixes the left view: left pixel (h, w) matches right pixel (h, w - dl); hence right pixel (h, w) matches left
 * pixel (h, w + dr).  A view is (s, own, other): left = (-1, dl, dr), right = (+1, dr, dl).
 *
 * Left-right consistency, per view, map k and pixel, with tau > 0 and dmax > 0:
 *   x      = w + s own(h, w)
 *   valid  iff own is finite, 0 <= own <= dmax, 0 <= x <= W - 1 and other[h, x0], other[h, x0 + 1] are both finite
 *   x0     = min(floor(x), W - 2);  t = x - x0;  oh = (1 - t) other[h, x0] + t other[h, x0 + 1]
 *   e      = |own - oh|  (0 where invalid)
 *   vis    = valid and e <= tau
 *   lr_v_k = sum of e over the valid pixels / max(N_valid, 1)
 *   loss   = sum_k weights[k] (lr_left_k + lr_right_k)
 * The term runs over all valid pixels, visible or not; the mask carries no gradient.  N_valid is a constant for the gradient and
 * sign(0) = 0.  Gradient of one view's term: into own(h, w)  sign(own - oh) (1 - s (other[x0 + 1] - other[x0])) / N; into other
 * -sign(own - oh) / N, times (1 - t) at x0 and t at x0 + 1.
 *
 * mode_lr_consistency_fwd: mask (2, K, B, H, W) bytes, 1 = visible, left view first; NULL = not wanted.  stats (2, K, MODE_LR_STATS)
 *   fp64 on the device: N_valid, the sum of e, N_visible, left view first.  loss: a device fp32 scalar.  One launch plus a one-block
 *   fold; fp32 terms accumulated in fp64 in a fixed order; no atomics: the same inputs give the same bits on any stream.
 *   workspace: device, 8-byte aligned, workspace_bytes >= mode_lr_consistency_workspace_bytes(K, B, H, W) (0 for refused sizes).
 * mode_lr_consistency_bwd: gdisp_l, gdisp_r (K, B, H, W) = gloss[0] * d loss / d disp, each element written once: its own view's
 *   direct part plus the other view's part, which a thread per target column gathers from the bounded window of source columns that
 *   can reach it (0 <= own <= dmax), in ascending column order.  `stats` as the forward wrote them for the same inputs.
 *
 * mode_selfsup_view_loss_fwd / _bwd: the loss of mode_photometric_loss_fwd / _bwd (mode_hip.h) seen from either camera and
 *   with an optional mask.  own_image supplies L and the smoothness edges, other_image is warped: x = w + s d with s = -1 for
 *   view 0 (left) and +1 for view 1 (right), d Rh / d d = s (R[x0 + 1] - R[x0]).  mask (K, B, H, W) bytes or NULL: a pixel is valid iff
 *   the warp's test holds and its mask byte is non-zero.  Everything else -- windows of nine valid pixels, moments, the smoothness
 *   term on every pixel masked or not, lam == 0, the reduction, stats (K x MODE_PHOTOMETRIC_STATS), the workspace of
 *   mode_photometric_loss_workspace_bytes -- is that entry's, and view 0 without a mask runs the very same kernels.
 *
 * Refusals, before any launch.  MODE_ERR_BAD_ARG: a NULL pointer other than the optional masks, K outside 1..4, B < 1, view outside
 * {0, 1}, tau or dmax not finite or not positive, W < 2 (consistency), H < 3 or W < 3 (view loss).  MODE_ERR_UNSUPPORTED: consistency
 * entries with B H >= 2^31 (one workgroup per row: the row index is 32-bit; offsets are 64-bit), W > MODE_LR_MAX_W (a row of both maps
 * and both views' records are staged in LDS) or dmax > W; view loss with 3 B H W >= 2^31 or W >= 2^24 (as mode_photometric_loss_fwd).
 * MODE_ERR_WORKSPACE: a missing, misaligned or short workspace. */
#ifndef MODE_HIP_SELFSUP_H_
#define MODE_HIP_SELFSUP_H_

#include "mode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODE_SELFSUP_VERSION 1
#define MODE_LR_MAX_MAPS 4
#define MODE_LR_STATS 3
#define MODE_LR_N_VALID 0
#define MODE_LR_SUM_E 1
#define MODE_LR_N_VISIBLE 2
#define MODE_LR_MAX_W 2048
#define MODE_SELFSUP_VIEW_STATS 4

typedef struct mode_lr_params {
  float tau, dmax;
  float weights[4]; /* wgt[k]; entries at and beyond K are ignored */
} mode_lr_params;

int mode_selfsup_version(void);
size_t mode_lr_consistency_workspace_bytes(int K, int B, int H, int W);
int mode_lr_consistency_fwd(const float* disp_l, const float* disp_r, int K, int B, int H, int W, const mode_lr_params* params,
                            void* workspace, size_t workspace_bytes, unsigned char* mask, double* stats, float* loss,
                            mode_stream_t stream);
int mode_lr_consistency_bwd(const float* disp_l, const float* disp_r, int K, int B, int H, int W, const mode_lr_params* params,
                            const double* stats, const float* gloss, float* gdisp_l, float* gdisp_r, mode_stream_t stream);
int mode_selfsup_view_loss_fwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask, int view,
                               int K, int B, int H, int W, const mode_photometric_params* params, void* workspace,
                               size_t workspace_bytes, double* stats, float* loss, mode_stream_t stream);
int mode_selfsup_view_loss_bwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask, int view,
                               int K, int B, int H, int W, const mode_photometric_params* params, const double* stats,
                               const float* gloss, float* gdisp, mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_SELFSUP_H_ */
