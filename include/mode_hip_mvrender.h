/* mode_hip_mvrender.h -- the sixth public header of libmode_hip.so: novel-view rendering, a panorama splatted through its depth map
 * into T other views.
 *
 * include/mode_hip_mvvis.h is frozen by its tests (MODE_MVVIS_VERSION 1 and its two launching entries); the entries added after it
 * are declared here.  mode_hip/_header.py reads this file on its own, so the constants are integer literals.  The conventions are the
 * first header's: plain C, device pointers unless stated, the stream is the last parameter and is named `stream`, every argument is
 * checked before any launch, no state is kept between calls, MODE_OK / MODE_ERR_* are the return codes and mode_last_error() has the
 * text.  This header has a version of its own, MODE_MVRENDER_VERSION / mode_mvrender_version().
 *
 * Inputs: image (F, C, H, W) fp32, 1 <= C <= MODE_MVR_MAX_CHANNELS, taken as it is (no mean or std: whatever the caller holds is
 * copied or interpolated); depth (F, H, W) fp32; poses: T x 12 doubles on the HOST, 1 <= T <= MODE_MVP_MAX_SOURCES -- a target view
 * is a source of include/mode_hip_mvphoto.h, X_t = A X + o; tol >= 0, a double; fill in {0, 1}; mode MODE_MVR_SPLAT or
 * MODE_MVR_RESAMPLE.  The validity rule of a reference pixel, Y, rho, u, v and the landing pixel (y, x) are exactly those of
 * include/mode_hip_mvvis.h, in fp64.  With them:
 *   z(f, t, y, x)      the minimum of rho over the valid pixels that land there, or +inf if none does
 *   owner(f, t, y, x)  the smallest index h W + w among the valid pixels that land there with rho == z (compared as fp64 bits), -1 if
 *                      none does
 *   fill == 0          a target pixel with finite z has class DIRECT, zc = z and from = owner; every other pixel has class NONE
 *   fill == 1          zn = the minimum of z over the 3 x 3 neighbourhood, rows modulo H and columns clipped to 0 .. W - 1.
 *                      DIRECT iff z is finite and z <= (1 + tol) zn (in fp64; 1 + tol is formed on the host): zc = z, from = owner.
 *                      Otherwise, if zn is finite, FILLED -- a hole, or a far surface seen through the cracks of a magnified near
 *                      one: zc = zn and from = the owner of the first neighbour that holds zn, scanned dy = -1, 0, 1 outside and
 *                      dx = -1, 0, 1 inside.  Otherwise NONE.
 *   range(f, t, y, x)  zc rounded to fp32, +inf for NONE
 *   index(f, t, y, x)  from, -1 for NONE
 *   out, SPLAT         out(f, t, c, y, x) = image(f, c, from), copied bit for bit; 0 for NONE
 *   out, RESAMPLE      for a pixel that is not NONE: X = A^T (zc n(y, x) - o) in fp64, r = |X|, and u_r, v_r from asin(X_x / r) and
 *                      atan2(X_y, X_z) by the formulas of include/mode_hip_mvphoto.h.  If r > 0 and 0 <= u_r <= W - 1:
 *                      x0 = min(floor u_r, W - 2), t = u_r - x0, y0 = floor v_r, q = v_r - y0, rows y0 mod H and (y0 + 1) mod H, t and q
 *                      rounded to fp32, top = (1 - t) r00 + t r01, bot likewise, out = (1 - q) top + q bot in fp32 in that order, and
 *                      hit gets MODE_MVR_HIT_RESAMPLED added.  Otherwise (beyond the reference's poles) the pixel takes SPLAT's value.
 *   hit(f, t, y, x)    the class, plus MODE_MVR_HIT_RESAMPLED where the pixel was resampled
 * No gradient is defined.
 *
 * mode_mv_render: out (F, T, C, H, W) fp32; hit (F, T, H, W) bytes; range (F, T, H, W) fp32 or NULL; index (F, T, H, W) int or NULL.
 *   Four launches whatever F, T and C are: the keys and the owners to all ones; the splat of include/mode_hip_mvvis.h; the owners,
 *   one thread per pixel-target pair, atomicMin of the pixel index where the pair's rho is its landing pixel's key; the resolve, one
 *   thread per target pixel and view.  Integer minima only: the same inputs give the same bits on any stream.  workspace: device,
 *   8-byte aligned, workspace_bytes >= mode_mvrender_workspace_bytes(T, F, H, W) (0 for refused sizes): with n = F T H W the keys
 *   (8 n), rho (8 n), the landing indices (4 n) and the owners (4 n), each part rounded up to 16 bytes.
 *
 * Refusals, before any launch: those of mode_mv_visibility with T for S (MODE_ERR_BAD_ARG: a NULL depth or poses, T outside 1 .. 8,
 * F < 1, H < 3, W < 3, a pose entry that is not finite, an A that is not orthonormal to 1e-9; MODE_ERR_UNSUPPORTED: 3 F T H W >= 2^31;
 * MODE_ERR_WORKSPACE: a missing, misaligned or short workspace), plus MODE_ERR_BAD_ARG: a NULL image, out or hit, C outside 1 .. 4, a
 * tol that is negative or not finite, fill or mode outside {0, 1}; and MODE_ERR_UNSUPPORTED: C F T H W >= 2^31. */
#ifndef MODE_HIP_MVRENDER_H_
#define MODE_HIP_MVRENDER_H_

#include "mode_hip_mvvis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODE_MVRENDER_VERSION 1

#define MODE_MVR_SPLAT 0
#define MODE_MVR_RESAMPLE 1
#define MODE_MVR_MAX_CHANNELS 4
#define MODE_MVR_HIT_NONE 0
#define MODE_MVR_HIT_DIRECT 1
#define MODE_MVR_HIT_FILLED 2
#define MODE_MVR_HIT_RESAMPLED 4

int mode_mvrender_version(void);
size_t mode_mvrender_workspace_bytes(int T, int F, int H, int W);
int mode_mv_render(const float* image, const float* depth, const double* poses, int T, int F, int C, int H, int W, double tol, int fill, int mode,
                   void* workspace, size_t workspace_bytes, float* out, unsigned char* hit, float* range, int* index, mode_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MODE_HIP_MVRENDER_H_ */
