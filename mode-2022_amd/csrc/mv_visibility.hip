// Z-buffer visibility of a fused depth map in S source views (include/mode_hip_mvvis.h): every pixel of the reference
// panorama is lifted by its depth and forward-projected into each source; the smallest range rho that lands on a source pixel is that
// source's depth there, and a reference pixel whose own rho exceeds (1 + tol) times what its landing place holds is hidden from that
// source.  By-product: the range map of every source rendered from the fused depth.
//
// Three launches whatever F and S are:
//   launch 1  the F S H W 64-bit keys = all ones (mode::fill_words)
//   launch 2  splat: one thread per reference pixel, the source loop inside.  The two fp64 sincos of the viewing direction are
//             computed once per pixel (pixel_dir), validity is that of the loss's own project<> (mv_photometric_internal.h), and the
//             key is the bit pattern of the fp64 rho -- positive doubles order as unsigned integers -- put with atomicMin on unsigned
//             long long as zbuffer_scatter_kernel (geometry.hip) does.  The thread leaves rho and the landing index (or -1) of each of
//             its pixel-source pairs in the workspace.
//   launch 3  resolve: one thread per pixel and source.  It reads back what the splat stored, so a pixel's own key compares equal by
//             construction; the minimum over 1 or 9 keys, the comparison in fp64, the vis byte; and, as a target pixel, zbuf.
// Integer minima do not depend on the order of arrival: the same inputs give the same bits on any stream.  The poses travel in the
// kernel arguments as in mv_photometric.hip.
#include "mode_hip_mvvis.h"
#include "mv_splat_internal.h"

namespace {

// n_px = F H W reference pixels; pair (f, s, h, w) has the index (f S + s) H W + h W + w, as vis has.
__global__ __launch_bounds__(NT) void mvvis_splat_kernel(const float* __restrict__ depth, Poses poses, int S, int H, int W, int n_px,
                                                         unsigned long long* __restrict__ keys, double* __restrict__ rho,
                                                         int* __restrict__ at) {
  const int HW = H * W;
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < n_px; idx += gridDim.x * NT) {
    const int f = idx / HW, r = idx - f * HW;
    const int h = r / W, w = r - h * W;
    const Dir n = pixel_dir(h, w, H, W);
    const float d = depth[idx];
    for (int sv = 0; sv < S; ++sv) {
      const int plane = (f * S + sv) * HW;  // < F S H W < 2^31
      const Landing l = land(d, n, poses.p[sv], H, W);
      if (l.at >= 0) atomicMin(keys + plane + l.at, (unsigned long long)__double_as_longlong(l.rho));
      rho[plane + r] = l.rho;
      at[plane + r] = l.at;
    }
  }
}

// n = F S H W pixel-source pairs.  one_tol = 1 + tol, formed in fp64 on the host.
__global__ __launch_bounds__(NT) void mvvis_resolve_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ rho,
                                                           const int* __restrict__ at, int H, int W, int n, double one_tol, int radius,
                                                           unsigned char* __restrict__ vis, float* __restrict__ zbuf) {
  const int HW = H * W;
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < n; idx += gridDim.x * NT) {
    const int plane = idx - idx % HW;
    const int a = at[idx];
    unsigned char seen = 0;
    if (a >= 0 && a < HW) {
      unsigned long long zmin = keys[plane + a];  // holds this pixel's own key or a smaller one
      if (radius) {
        const int y = a / W, x = a - y * W;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          int yy = y + dy;
          yy = yy < 0 ? yy + H : (yy >= H ? yy - H : yy);
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx > W - 1) continue;
            const unsigned long long k = keys[plane + yy * W + xx];
            zmin = k < zmin ? k : zmin;
          }
        }
      }
      seen = rho[idx] <= one_tol * __longlong_as_double((long long)zmin) ? 1 : 0;
    }
    vis[idx] = seen;
    if (zbuf) {
      const unsigned long long k = keys[idx];
      zbuf[idx] = k == kEmpty ? __builtin_inff() : (float)__longlong_as_double((long long)k);
    }
  }
}

}  // namespace

// land(), the empty key, grid_for() and part() are mv_splat_internal.h's, shared with mv_render.hip.  The three parts of the
// workspace, each 16-byte aligned: keys (8 n), rho (8 n), landing indices (4 n).

extern "C" int mode_mvvis_version(void) { return MODE_MVVIS_VERSION; }

extern "C" size_t mode_mvvis_workspace_bytes(int S, int F, int H, int W) {
  if (S < 1 || S > kMaxS || F < 1 || H < 3 || W < 3 || 3ll * F * S * H * W >= (1ll << 31)) return 0;
  const size_t n = (size_t)F * S * H * W;
  return 2 * part(8 * n) + part(4 * n);
}

extern "C" int mode_mv_visibility(const float* depth, const double* poses, int S, int F, int H, int W, double tol, int radius,
                                  void* workspace, size_t workspace_bytes, unsigned char* vis, float* zbuf, mode_stream_t stream) {
  const char* who = "mode_mv_visibility";
  MODE_REQUIRE(vis, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  // The family's own checks of the sizes and the poses, in the family's words.  This entry reads no image and no colour parameters:
  // the depth stands in for the two images, and the bound of the loss these masks are for, 3 F S H W < 2^31, holds here as well
  // (the indices of this file need F S H W < 2^31).
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  const mode_photometric_params no_colour = {};
  int rc = check_common(who, depth, depth, depth, poses, S, F, H, W, &no_colour, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(std::isfinite(tol) && tol >= 0.0, MODE_ERR_BAD_ARG, "%s: tol = %g must be finite and >= 0", who, tol);
  MODE_REQUIRE(radius == 0 || radius == 1, MODE_ERR_BAD_ARG, "%s: radius = %d (0 or 1)", who, radius);
  rc = check_workspace(who, workspace, workspace_bytes, mode_mvvis_workspace_bytes(S, F, H, W));
  if (rc != MODE_OK) return rc;
  const size_t n = (size_t)F * S * H * W;
  char* base = static_cast<char*>(workspace);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
  double* rho = reinterpret_cast<double*>(base + part(8 * n));
  int* at = reinterpret_cast<int*>(base + 2 * part(8 * n));
  hipStream_t st = mode::as_stream(stream);
  rc = mode::fill_words(keys, 0xffffffffu, 2 * n, st, who);  // all keys = +inf (a kernel, not hipMemsetAsync: common.h)
  if (rc != MODE_OK) return rc;
  const int n_px = F * H * W;
  hipLaunchKernelGGL(mvvis_splat_kernel, dim3(grid_for(n_px)), dim3(NT), 0, st, depth, ps, S, H, W, n_px, keys, rho, at);
  hipLaunchKernelGGL(mvvis_resolve_kernel, dim3(grid_for((long long)n)), dim3(NT), 0, st, keys, rho, at, H, W, (int)n, 1.0 + tol, radius,
                     vis, zbuf);
  return mode::check_launch(who);
}
