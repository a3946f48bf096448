// The multi-view hand-off between the two networks: the six disparity / confidence pairs of F Deep360 frames -> the
// fusion network's input, in three launches whatever F is.  For frame f and pair p (order 12, 13, 14, 23, 24, 34) it computes what
// utils.geometry.disp2depth_gpu(disp[f, p], conf[f, p], PAIR[p]) computes, bit for bit, from the same per-pixel arithmetic
// (geometry_internal.h):
//   12        the sine rule                                            (mode_disp2depth)
//   13, 14    the sine rule + rotateCassini, i.e. the bilinear border gather on the cached rotation grid, the depth of each of the
//             four corners formed on the fly from the disparity          (mode_disp2depth + mode_grid_sample_border, C = 2)
//   23 24 34  the sine rule + depthViewTransWithConf with its z-buffer   (mode_disp2depth + mode_depth_view_trans)
// and writes out[f, 2p] = depth, out[f, 2p + 1] = q(confidence) -- ModeFusion's channel interleave -- or out[f, p] = depth alone
// (MODE_MV_DEPTH_ONLY, the Baseline's input).  q is the identity, or with MODE_MV_CONF_PNG the 8-bit PNG round trip of the
// reference's export (conf_png below).
//   launch 1  every key plane of the three view-transformed maps of every frame = +inf (mode::fill_words)
//   launch 2  one thread per SOURCE pixel of the F x 6 disparity maps
//   launch 3  one thread per TARGET pixel of the F x 3 view-transformed maps
#include "common.h"
#include "geometry_internal.h"

namespace {

namespace geom = mode::geom;
constexpr int NT = 256;

struct MvArgs {
  float baseline[6];       // per pair
  geom::ViewXform xf[3];   // pairs 23, 24, 34
  int png;                 // MODE_MV_CONF_PNG
  int oc;                  // output channels per pair: 2 (depth, confidence) or 1 (MODE_MV_DEPTH_ONLY)
};

// The reference writes the confidence as an 8-bit PNG (cv2.imwrite(conf * 255): float32 product, saturate_cast<uchar> = round half
// to even and clamp) and reads it back as / 255.0 in float64, cast to float32 by the fusion loader.  NaN reads back as 0.
__device__ __forceinline__ float conf_png(float c) {
  const float r = fminf(255.f, fmaxf(0.f, rintf(c * 255.0f)));
  return (float)((double)r / 255.0);
}

__device__ __forceinline__ float conf_out(const MvArgs& a, float c) { return a.png ? conf_png(c) : c; }

__global__ __launch_bounds__(NT) void mv_pairs_kernel(const float* __restrict__ disp, const float* __restrict__ conf,
                                                      const float* __restrict__ rot_grids, const float* __restrict__ trig,
                                                      unsigned long long* __restrict__ keys, float* __restrict__ out, int F, int H,
                                                      int W, MvArgs a) {
  const long long hw = (long long)H * W;
  const long long total = (long long)F * 6 * hw;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const long long plane = idx / hw;  // f * 6 + p
    const long long pix = idx - plane * hw;
    const int p = (int)(plane % 6);
    const long long f = plane / 6;
    const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
    const float* dp = disp + plane * hw;
    const float* cp = conf + plane * hw;
    float* od = out + plane * a.oc * hw + pix;  // out[f, oc * p] (+ hw: out[f, 2p + 1])
    const float baseline = a.baseline[p];
    if (p == 0) {
      od[0] = geom::sine_rule_depth(dp[pix], j, W, baseline);
      if (a.oc == 2) od[hw] = conf_out(a, cp[pix]);
    } else if (p < 3) {
      // rotateCassini by pitch pi/2 (13) or pi/4 (14): grid (2, H, W, 2), the sampled source the sine-rule depth of the same map
      const float2 g = reinterpret_cast<const float2*>(rot_grids)[(p - 1) * hw + pix];
      const geom::Bilinear b = geom::bilinear_border(g, H, W);
      od[0] = geom::bilinear_sum(b, [=](int y, int x) { return geom::sine_rule_depth(dp[(long long)y * W + x], x, W, baseline); });
      if (a.oc == 2) od[hw] = conf_out(a, geom::bilinear_sum(b, [=](int y, int x) { return cp[(long long)y * W + x]; }));
    } else {
      // depthViewTransWithConf: this source pixel's bid for its target in the key plane of (f, p)
      const geom::ViewXform& xf = a.xf[p - 3];
      double r2;
      long long tgt;
      if (geom::project_pixel(geom::sine_rule_depth(dp[pix], j, W, baseline), trig[j], trig[W + j], trig[2 * W + i],
                              trig[2 * W + H + i], xf, H, W, r2, tgt))
        atomicMin(keys + (f * 3 + (p - 3)) * hw + tgt, geom::zkey(r2, pix, hw));
    }
  }
}

__global__ __launch_bounds__(NT) void mv_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ conf,
                                                        float* __restrict__ out, int F, int H, int W, MvArgs a) {
  const long long hw = (long long)H * W;
  const long long total = (long long)F * 3 * hw;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const long long kp = idx / hw;  // f * 3 + (p - 3)
    const long long pix = idx - kp * hw;
    const long long plane = (kp / 3) * 6 + 3 + kp % 3;  // f * 6 + p
    const float2 vc = geom::resolve_key(keys[idx], conf + plane * hw, hw);
    float* od = out + plane * a.oc * hw + pix;
    od[0] = vc.x;
    if (a.oc == 2) od[hw] = conf_out(a, vc.y);
  }
}

int grid_for(long long n) { return (int)std::min<long long>(mode::cdiv(n, NT), 8LL * kNumCU); }

}  // namespace

extern "C" size_t mode_multiview_handoff_workspace_bytes(int F, int H, int W) {
  return F > 0 && H > 0 && W > 0 ? 3 * (size_t)F * H * W * sizeof(unsigned long long) : 0;
}

extern "C" int mode_multiview_handoff(const float* disp, const float* conf, int F, int H, int W, const float* baselines6,
                                      const float* rot_grids, const float* trig, const double* xforms, int flags, float* out,
                                      void* workspace, mode_stream_t stream) {
  MODE_REQUIRE(F >= 0 && H > 0 && W > 0 && 3LL * F * H * W < (1LL << 31), MODE_ERR_BAD_ARG, "mode_multiview_handoff: bad size %d x %dx%d",
               F, H, W);
  MODE_REQUIRE((flags & ~(MODE_MV_CONF_PNG | MODE_MV_DEPTH_ONLY)) == 0, MODE_ERR_BAD_ARG, "mode_multiview_handoff: unknown flags 0x%x",
               flags);
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(disp && conf && baselines6 && rot_grids && trig && xforms && out, MODE_ERR_BAD_ARG, "mode_multiview_handoff: null pointer");
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(rot_grids) & 7) == 0, MODE_ERR_BAD_ARG, "mode_multiview_handoff: rotation grids must be 8-byte aligned");
  MODE_REQUIRE(workspace, MODE_ERR_WORKSPACE, "mode_multiview_handoff: workspace required");
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MODE_ERR_WORKSPACE, "mode_multiview_handoff: unaligned workspace");
  MvArgs a;
  for (int p = 0; p < 6; ++p) a.baseline[p] = baselines6[p];
  for (int v = 0; v < 3; ++v) {
    for (int k = 0; k < 9; ++k) a.xf[v].R[k] = xforms[12 * v + k];
    for (int k = 0; k < 3; ++k) a.xf[v].t[k] = xforms[12 * v + 9 + k];
  }
  a.png = (flags & MODE_MV_CONF_PNG) ? 1 : 0;
  a.oc = (flags & MODE_MV_DEPTH_ONLY) ? 1 : 2;
  hipStream_t st = mode::as_stream(stream);
  const long long hw = (long long)H * W;
  // all keys = +inf (a kernel, not hipMemsetAsync: common.h)
  int frc = mode::fill_words(workspace, 0xffffffffu, 2 * 3 * (size_t)F * hw, st, "mode_multiview_handoff");
  if (frc != MODE_OK) return frc;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(mv_pairs_kernel, dim3(grid_for(6LL * F * hw)), dim3(NT), 0, st, disp, conf, rot_grids, trig, keys, out, F, H, W, a);
  hipLaunchKernelGGL(mv_resolve_kernel, dim3(grid_for(3LL * F * hw)), dim3(NT), 0, st, keys, conf, out, F, H, W, a);
  return mode::check_launch("mode_multiview_handoff");
}
