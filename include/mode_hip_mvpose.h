/* mode_hip_mvpose.h -- the fourth public header of libmode_hip.so: the gradient of the multi-view reprojection loss with respect to
 * the sources' poses, for the self-calibration of a rig.
 *
 * include/mode_hip_mvphoto.h is frozen by its tests (MODE_MVPHOTO_VERSION 1 and its two launching entries); the entry added after it
 * is declared here.  mode_hip/_header.py reads this file on its own, so the constants are integer literals.  The conventions are the
 * first header's: plain C, device pointers unless stated, the stream is the last parameter and is named `stream`, every argument is
 * checked before any launch, no state is kept between calls, MODE_OK / MODE_ERR_* are the return codes and mode_last_error() has the
 * text.  This header has a version of its own, MODE_MVPOSE_VERSION / mode_mvpose_version().
 *
 * The notation, the inputs and the loss are those of mode_hip_mvphoto.h: ref, src, depth, poses (HOST memory, S x 12 doubles, row-major
 * [A | o] per source), params; win and stats as mode_mvphoto_loss_fwd wrote them for the same inputs.  For source s, pixel
 * p = (f, h, w) with depth D and direction n:
 *   m = A n;  Y = D m + o;  rho^2 = |Y|^2;  u, v as in mode_hip_mvphoto.h
 *   a_c(p, s)  = d (sum of the window minima) / d Ih_{s,c}(p): the shares of the up to nine windows that contain p and were won by s,
 *                plus the L1 term of p's own window if s won it -- the per-channel factor mode_mvphoto_loss_bwd multiplies the slope with
 *   Ih_u,c, Ih_v,c  the bilinear's two partial slopes;  G_u = sum_c a_c Ih_u,c,  G_v = sum_c a_c Ih_v,c  (fp32)
 *   grad_Y u   = -(W / pi) (e_x rho^2 - Y_x Y) / (rho^2 sqrt(Y_y^2 + Y_z^2))
 *   grad_Y v   = -(H / 2 pi) (0, Y_z, -Y_y) / (Y_y^2 + Y_z^2)             (fp64; with Y moved along m: du / dD, dv / dD of that header)
 *   g_Y(p, s)  = G_u grad_Y u + G_v grad_Y v, formed in fp64 from the fp32 G_u, G_v; 0 where p is invalid for s
 *   gposes[s]  = (gloss[0] / max(N, 1)) sum_p g_Y(p, s) (x) (D n_x, D n_y, D n_z, 1)
 * a 3 x 4 table per source, row-major like poses: d loss / d A in the first three columns (A taken as nine free numbers) and
 * d loss / d o in the fourth.  N and win are constants of the gradient; the smoothness term does not depend on the poses.
 *
 * Two properties of this gradient:
 *   ONE-SIDED WHERE v IS AN INTEGER AND THE POSE MOVES v.  The bilinear is continuous in v but not differentiable at integer v: floor
 *   chooses between the rows (y0, y0 + 1) and (y0 - 1, y0), and the two slopes differ.  dv / dD is exactly 0 there, so the gradient to
 *   the depth never saw it; the gradient to the pose does.  With exactly rectified poses (the right camera of the reference's own
 *   pair: v == h at every pixel) d loss / d o_y and d loss / d o_z are the derivative on the side floor chose, and differ from a
 *   central difference by 10 to 30 % of max |g|.  With generic poses it is the derivative.  (utils.rig_refine gives the identity pair
 *   no parameters, so that pair is not differentiated.)
 *   A SOURCE THAT WINS NO WINDOW GETS AN EXACTLY ZERO ROW: the loss takes the minimum per window.  A miscalibrated source that loses
 *   against a well-calibrated one nearly everywhere converges slowly or not at all: calibrate a source at a time, or only sources
 *   that are comparably off.
 *
 * mode_mvpose_grad: gposes: device, S x 12 fp64, every element written on every call.  One launch (one workgroup per 16 x 32 tile, the
 *   source loop inside) plus a fold of one block per source; fp64 sums in a fixed order, no atomics: the same inputs give the same bits
 *   on any stream.  workspace: device, 8-byte aligned, workspace_bytes >= mode_mvpose_workspace_bytes(S, F, H, W) (0 for refused sizes).
 *
 * Refusals, before any launch: those of mode_mvphoto_loss_bwd (MODE_ERR_BAD_ARG: a NULL pointer, S outside 1 .. 8, F < 1, H < 3, W < 3,
 * a pose entry that is not finite, an A that is not orthonormal to 1e-9; MODE_ERR_UNSUPPORTED: 3 F S H W >= 2^31) and
 * MODE_ERR_WORKSPACE: a missing, misaligned or short workspace. */
#ifndef MODE_HIP_MVPOSE_H_
#define MODE_HIP_MVPOSE_H_

#include "mode_hip_mvphoto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODE_MVPOSE_VERSION 1

int mode_mvpose_version(void);
size_t mode_mvpose_workspace_bytes(int S, int F, int H, int W);
int mode_mvpose_grad(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                     const mode_photometric_params* params, const unsigned char* win, const double* stats, const float* gloss,
                     void* workspace, size_t workspace_bytes, double* gposes, mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_MVPOSE_H_ */
