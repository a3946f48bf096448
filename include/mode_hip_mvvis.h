/* mode_hip_mvvis.h -- the fifth public header of libmode_hip.so: z-buffer visibility masks of a fused depth map per source view, and
 * the multi-view reprojection loss restricted to them.
 *
 * include/mode_hip_mvpose.h is frozen by its tests (MODE_MVPOSE_VERSION 1 and its launching entry); the entries added after it are
 * declared here.  mode_hip/_header.py reads this file on its own, so the constants are integer literals.  The conventions are the
 * first header's: plain C, device pointers unless stated, the stream is the last parameter and is named `stream`, every argument is
 * checked before any launch, no state is kept between calls, MODE_OK / MODE_ERR_* are the return codes and mode_last_error() has the
 * text.  This header has a version of its own, MODE_MVVIS_VERSION / mode_mvvis_version().
 *
 * The per-window minimum of mode_hip_mvphoto.h chooses among whatever the sources show: where a surface is hidden from a source, that
 * source still samples the occluder's colour there and wins the window whenever that colour happens to match.  The fused depth,
 * forward-projected into a source, is a depth map of that source; a pixel whose own range to the source's centre exceeds what that
 * map holds at its landing place is hidden there.
 *
 * Inputs: depth (F, H, W) fp32; poses: S x 12 doubles on the HOST, 1 <= S <= MODE_MVP_MAX_SOURCES; tol >= 0, a double; radius in
 * {0, 1}.  Notation, angles at pixel centres, Y = depth (A n) + o, rho = |Y|, u, v and the validity rule are exactly those of
 * include/mode_hip_mvphoto.h, in fp64.
 *   Landing pixel of a valid (f, s, h, w): x = floor(u + 1/2), y = floor(v + 1/2) mod H.  u lies in [0, W - 1], so x does too.
 *   z(f, s, y, x)     the minimum of rho over the valid pixels of frame f that land on (y, x) in source s, or +inf if none does
 *   zmin              of a landing pixel: z there when radius == 0; when radius == 1 the minimum of z over the 3 x 3 neighbourhood,
 *                     rows modulo H and columns clipped to 0 .. W - 1
 *   vis(f, s, h, w)   = 1 iff the pixel is valid for s and rho <= (1 + tol) * zmin(landing pixel); the comparison is in fp64, and
 *                     1 + tol is formed in fp64
 *   zbuf(f, s, y, x)  z rounded to fp32
 * A pixel's own key is in its landing pixel, so with any tol >= 0 a pixel that is alone there is visible.  The masks are constants
 * of every gradient.
 *
 * ON THE +-pi SEAM THE ROW IS ONE-SIDED.  v + 1/2 = (pi - theta') H / (2 pi) is an integer where theta' is a multiple of 2 pi / H;
 * nearest rounding makes that a row boundary, and floor chooses the upper row.  With odd H and A = I the middle row has n_y = 0
 * exactly and theta' sits on the seam +-pi, where the sign of a rounding error in Y_y chooses between row 0 and row H: both are row 0
 * modulo H there, but one row further the choice is between two different rows.  A float64 restatement agrees with the kernel on
 * every landing pixel only where no valid u + 1/2 or v + 1/2 is an integer (tests/test_mvvis_host.py asserts a margin of 1e-9 for
 * its cases, which have even H).
 *
 * Masked loss.  The loss of mode_hip_mvphoto.h with one change: a pixel is valid for source s iff it is valid there AND
 * vis(f, s, h, w) != 0.  win, N, photo, the statistics and the gradient rules are otherwise word for word.  mode_mvphoto_loss_bwd
 * and mode_mvpose_grad take the masked forward's win and stats as they are: a window won by s contains only pixels that are valid and
 * visible for s.
 *
 * mode_mv_visibility: vis (F, S, H, W) bytes, 0 or 1; zbuf (F, S, H, W) fp32 or NULL.  Three launches whatever F and S are: the keys
 *   to all ones; a splat, one thread per reference pixel with the source loop inside, atomicMin on the bit pattern of the fp64 rho
 *   (positive doubles order as unsigned integers); a resolve, one thread per pixel and source.  Integer minima do not depend on the
 *   order of arrival: the same inputs give the same bits on any stream.  workspace: device, 8-byte aligned, workspace_bytes >=
 *   mode_mvvis_workspace_bytes(S, F, H, W) (0 for refused sizes): the keys, and rho and the landing index of every pixel-source pair.
 * mode_mvphoto_loss_fwd_masked: the arguments of mode_mvphoto_loss_fwd plus vis (F, S, H, W) bytes, read as != 0; the workspace is
 *   that entry's (mode_mvphoto_workspace_bytes).
 *
 * Refusals, before any launch: those of mode_mvphoto_loss_fwd (MODE_ERR_BAD_ARG: a NULL pointer other than zbuf, S outside 1 .. 8,
 * F < 1, H < 3, W < 3, a pose entry that is not finite, an A that is not orthonormal to 1e-9; MODE_ERR_WORKSPACE: a missing,
 * misaligned or short workspace; MODE_ERR_UNSUPPORTED: 3 F S H W >= 2^31), plus MODE_ERR_BAD_ARG: a tol that is negative or not
 * finite, a radius outside {0, 1}.  F S H W >= 2^31, which the 32-bit indices of mode_mv_visibility could not address, is refused
 * with the loss's own bound: the masks are for that loss. */
#ifndef MODE_HIP_MVVIS_H_
#define MODE_HIP_MVVIS_H_

#include "mode_hip_mvphoto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODE_MVVIS_VERSION 1

int mode_mvvis_version(void);
size_t mode_mvvis_workspace_bytes(int S, int F, int H, int W);
int mode_mv_visibility(const float* depth, const double* poses, int S, int F, int H, int W, double tol, int radius, void* workspace,
                       size_t workspace_bytes, unsigned char* vis, float* zbuf, mode_stream_t stream);
int mode_mvphoto_loss_fwd_masked(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                                 const mode_photometric_params* params, void* workspace, size_t workspace_bytes,
                                 const unsigned char* vis, unsigned char* win, double* stats, float* loss, mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_MVVIS_H_ */
