/* mode_hip_mvphoto.h -- the third public header of libmode_hip.so: multi-view reprojection loss of a fused depth map.
 *
 * include/mode_hip.h and include/mode_hip_selfsup.h are frozen by their tests (ABI 31; MODE_SELFSUP_VERSION 1 and its four launching
 * entries); entries added after them are declared here.  mode_hip/_header.py reads this file on its own, exactly as it reads the other
 * two, so the constants below are integer literals.  The conventions are the first header's: plain C, device pointers unless stated,
 * the stream is the last parameter and is named `stream`, every argument is checked before any launch, no state is kept between calls,
 * MODE_OK / MODE_ERR_* are the return codes and mode_last_error() has the text.  This header has a version of its own,
 * MODE_MVPHOTO_VERSION / mode_mvphoto_version().
 *
 * ref (F, 3, H, W), src (F, S, 3, H, W), depth (F, H, W), all fp32 Cassini images of one size; 1 <= S <= MODE_MVP_MAX_SOURCES.  The
 * images are normalised: L = ref * std + mean, and the sources likewise (params->mean, params->std).  H is Cassini's periodic axis; W
 * runs pole to pole and does not wrap.  poses: HOST memory, S x 12 doubles read during the call, row-major [A | o] (3 x 4) per source:
 * a point X in the axes of the reference view has the coordinates A X + o in the Cassini frame of source s.
 *
 * Pixel (h, w) looks along n = (sin phi, cos phi sin theta, cos phi cos theta) with theta = pi - (h + 1/2) 2 pi / H and
 * phi = pi/2 - (w + 1/2) pi / W: angles at pixel centres, on both sides of the warp.  For one pixel and source:
 *   Y = depth (A n) + o;  rho = |Y|;  phi' = asin(Y_x / rho);  theta' = atan2(Y_y, Y_z)
 *   u = (pi/2 - phi') W / pi - 1/2;  v = (pi - theta') H / (2 pi) - 1/2
 *   valid iff depth is finite and > 0, rho > 0 and 0 <= u <= W - 1
 *   x0 = min(floor(u), W - 2), t = u - x0;  y0 = floor(v), q = v - y0;  rows y0 mod H and (y0 + 1) mod H
 *   Ih_s = the bilinear value of the de-normalised source (0 and without a gradient where invalid)
 * u, v and their slopes are computed in fp64 and rounded to fp32 at t, q and the slopes; everything after is fp32.
 * pe_s of a window is the pe of mode_photometric_loss_fwd (mode_hip.h) between L and Ih_s: 3x3 windows, rows modulo H,
 * centre columns 1 .. W - 2, centred biased moments, unclamped ssim, alpha (1 - ssim) / 2 + (1 - alpha) |L - Ih| averaged over the
 * channels; the window is valid for s iff its nine pixels are.
 *   win(h, w)  the smallest s that attains min_s pe_s over the sources whose window is valid; 255 if none is (and at columns 0, W - 1)
 *   photo      sum of the minima / max(N, 1), N = the number of windows with win != 255 (a constant for the gradient)
 *   smooth     mean over F H (W - 1) column neighbours of |log D(h, w + 1) - log D(h, w)| exp(-beta mean_c |L_c(h, w + 1) - L_c(h, w)|)
 *              + the mean over F H W row neighbours (h + 1 modulo H) of the same; a pair with a depth that is not finite and > 0
 *              contributes 0 and gets no gradient
 *   loss       photo + lam smooth; lam == 0 leaves the smoothness term out altogether; sign(0) = 0
 * The gradient goes into depth only, and from a window to its winning source only:
 *   m = A n;  d phi' / dD = (m_x rho^2 - Y_x (Y . m)) / (rho^2 sqrt(Y_y^2 + Y_z^2));  d theta' / dD = (m_y Y_z - m_z Y_y) / (Y_y^2 + Y_z^2)
 *   du / dD = -(W / pi) d phi' / dD;  dv / dD = -(H / 2 pi) d theta' / dD;  d Ih / dD = the bilinear's two partial slopes times these.
 *
 * mode_mvphoto_loss_fwd: win (F, H, W) bytes; stats MODE_MVP_STATS fp64 on the device: N, the sum of the minima, the two smoothness
 *   sums (columns, rows), then the number of windows won by each of the MODE_MVP_MAX_SOURCES sources; loss: a device fp32 scalar.  One
 *   launch plus a one-block fold; fp32 terms accumulated in fp64 in a fixed order, no atomics: the same inputs give the same bits on any
 *   stream.  workspace: device, 8-byte aligned, workspace_bytes >= mode_mvphoto_workspace_bytes(S, F, H, W) (0 for refused sizes).
 * mode_mvphoto_loss_bwd: gdepth (F, H, W) = gloss[0] * d loss / d depth, each element written once (a gather; no scatter).  win and
 *   stats as the forward wrote them for the same inputs.
 *
 * Refusals, before any launch.  MODE_ERR_BAD_ARG: a NULL pointer, S outside 1 .. 8, F < 1, H < 3, W < 3, a pose entry that is not
 * finite, an A that is not orthonormal to 1e-9 (max |A A^T - I|).  MODE_ERR_UNSUPPORTED: 3 F S H W >= 2^31 (offsets into the sources
 * are 32-bit).  MODE_ERR_WORKSPACE: a missing, misaligned or short workspace. */
#ifndef MODE_HIP_MVPHOTO_H_
#define MODE_HIP_MVPHOTO_H_

#include "mode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODE_MVPHOTO_VERSION 1
#define MODE_MVP_MAX_SOURCES 8
#define MODE_MVP_STATS 12
#define MODE_MVP_N 0
#define MODE_MVP_SUM_MIN 1
#define MODE_MVP_SUM_SMOOTH_X 2
#define MODE_MVP_SUM_SMOOTH_Y 3
#define MODE_MVP_WINS 4
#define MODE_MVP_NO_WINNER 255

int mode_mvphoto_version(void);
size_t mode_mvphoto_workspace_bytes(int S, int F, int H, int W);
int mode_mvphoto_loss_fwd(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                          const mode_photometric_params* params, void* workspace, size_t workspace_bytes, unsigned char* win,
                          double* stats, float* loss, mode_stream_t stream);
int mode_mvphoto_loss_bwd(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                          const mode_photometric_params* params, const unsigned char* win, const double* stats, const float* gloss,
                          float* gdepth, mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_MVPHOTO_H_ */
