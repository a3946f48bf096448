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
// reference's export (conf_png, multiview_internal.h).
//   launch 1  every key plane of the three view-transformed maps of every frame = +inf (mode::fill_words)
//   launch 2  one thread per SOURCE pixel of the F x 6 disparity maps
//   launch 3  one thread per TARGET pixel of the F x 3 view-transformed maps
#include "common.h"
#include "geometry_internal.h"
#include "multiview_internal.h"

namespace {

namespace geom = mode::geom;
using namespace mode::mv;  // conf_png, sine_rule_raw, sine_rule_slope (shared with multiview_rig.hip)
constexpr int NT = 256;

struct MvArgs {
  float baseline[6];       // per pair
  geom::ViewXform xf[3];   // pairs 23, 24, 34
  int png;                 // MODE_MV_CONF_PNG
  int oc;                  // output channels per pair: 2 (depth, confidence) or 1 (MODE_MV_DEPTH_ONLY)
};

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

// ---------------------------------------------------------------------------------------------------------------------
// The gradient of the hand-off's depth channels with respect to the disparities (mode_multiview_handoff_bwd, DESIGN 12 "Gradient").
// The confidence channels are not read there.  With q the identity they are linear in the confidence maps, and FULL
// (mode_multiview_handoff_bwd_full, DESIGN 12 "Gradient of the confidence") writes that gradient beside gdisp in the same two launches:
// the copy (12), the same walk over the adjoint list with the confidence channel's upstream gradient (13, 14; for EVERY source: the
// confidence does not depend on the disparity), the target's gradient to the winner of its key (23, 24, 34; capped winners and
// winners without a slope included: geom::resolve_key passes their confidence on).  Under MODE_MV_CONF_PNG q is piecewise constant
// and there is no such gradient: the entry refuses it.
//   launch A  one thread per SOURCE pixel of the F x 6 maps: planes 12, 13, 14 get their value, planes 23, 24, 34 get +0
//   launch B  one thread per TARGET pixel of the F x 3 view-transformed maps: the winner of its key gets the target's gradient
// A source bids for one target, so it wins at most one: launch B's stores never collide, and no sum is formed with atomics.

template <bool FULL>
__global__ __launch_bounds__(NT) void mv_bwd_sources_kernel(const float* __restrict__ disp, const float* __restrict__ gout,
                                                            const int* __restrict__ rowptr, const int* __restrict__ target,
                                                            const float* __restrict__ weight, int n_adj, float* __restrict__ gdisp,
                                                            int F, int H, int W, MvArgs a, float* __restrict__ gconf) {
  const long long hw = (long long)H * W;
  const long long total = (long long)F * 6 * hw;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const long long plane = idx / hw;  // f * 6 + p
    const long long pix = idx - plane * hw;
    const int p = (int)(plane % 6);
    float g = 0.f, gc = 0.f;  // pairs 23, 24, 34: launch B fills the winners in
    if (p < 3) {
      const int j = (int)(pix % W);
      const float s = sine_rule_slope(disp[idx], j, W, a.baseline[p]);
      const float* gd = gout + plane * a.oc * hw;  // gout[f, oc * p]; FULL (oc = 2): gd + hw = gout[f, 2p + 1]
      if (p == 0) {
        if (s != 0.f) g = gd[pix] * s;
        if (FULL) gc = gd[hw + pix];
      } else if (FULL || s != 0.f) {
        // the (target, weight) entries of the rotation grid whose corner this source is, in the list's stored order
        const int* rp = rowptr + (p - 1) * (hw + 1) + pix;
        const int k0 = max(rp[0], 0), k1 = min(rp[1], n_adj);
        float acc = 0.f;
        for (int k = k0; k < k1; ++k) {
          const int t = target[k];
          if ((unsigned)t < (unsigned)hw) {
            acc += weight[k] * gd[t];
            if (FULL) gc += weight[k] * gd[hw + t];
          }
        }
        if (s != 0.f) g = s * acc;
      }
    }
    gdisp[idx] = g;
    if (FULL) gconf[idx] = gc;
  }
}

template <bool FULL>
__global__ __launch_bounds__(NT) void mv_bwd_winners_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ disp,
                                                            const float* __restrict__ gout, const float* __restrict__ trig,
                                                            float* __restrict__ gdisp, int F, int H, int W, MvArgs a,
                                                            float* __restrict__ gconf) {
#pragma clang fp contract(off)  // r2 as geom::project_pixel rounds it
  const long long hw = (long long)H * W;
  const long long total = (long long)F * 3 * hw;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const unsigned long long k = keys[idx];
    if (k == ~0ull) continue;  // no source reached this target
    const float v = __uint_as_float((unsigned)(k >> 32));
    // geom::resolve_key: capped (strictly above; its 100000 -> 0 rule lies above the cap too): a constant depth.  Its confidence is
    // the winner's all the same, so FULL decodes the winner first.
    if (!FULL && v > 1000.f) continue;
    const unsigned lo = (unsigned)(k & 0xffffffffull);
    const long long src = (lo & 0x80000000u) ? (long long)(lo & 0x7fffffffu) : hw - 1 - (long long)lo;
    if (src < 0 || src >= hw) continue;  // (not a key of this size's forward)
    const long long kp = idx / hw;  // f * 3 + (p - 3)
    const long long pix = idx - kp * hw;
    const int v3 = (int)(kp % 3);
    const long long plane = (kp / 3) * 6 + 3 + v3;  // f * 6 + p
    if (FULL) {
      gconf[plane * hw + src] = gout[(plane * 2 + 1) * hw + pix];
      if (v > 1000.f) continue;
    }
    const int i = (int)(src / W), j = (int)(src - (long long)i * W);
    const float baseline = a.baseline[3 + v3];
    const float d = disp[plane * hw + src];
    const float s = sine_rule_slope(d, j, W, baseline);
    if (s == 0.f) continue;
    // r2 = |r1 dir - t| (R is orthonormal), so d r2 / d r1 = (r1 - dir . t) / r2 with |dir| = 1
    const geom::ViewXform& xf = a.xf[v3];
    const float r1 = geom::sine_rule_depth(d, j, W, baseline);
    const float sin_phi = trig[j], cos_phi = trig[W + j], sin_theta = trig[2 * W + i], cos_theta = trig[2 * W + H + i];
    const float rc = r1 * cos_phi;
    const float x1 = r1 * sin_phi, y1 = rc * sin_theta, z1 = rc * cos_theta;
    const double ax = (double)x1 - xf.t[0], ay = (double)y1 - xf.t[1], az = (double)z1 - xf.t[2];
    const double r2 = sqrt(ax * ax + ay * ay + az * az);
    const double dir_t = (double)sin_phi * xf.t[0] + (double)(cos_phi * sin_theta) * xf.t[1] + (double)(cos_phi * cos_theta) * xf.t[2];
    const float slope = (float)(((double)r1 - dir_t) / r2);
    gdisp[plane * hw + src] = gout[plane * a.oc * hw + pix] * slope * s;
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

namespace {

// mode_multiview_handoff_bwd (FULL = false, gconf unread) and mode_multiview_handoff_bwd_full: the same checks and the same two launches
template <bool FULL>
int handoff_bwd_run(const char* who, const float* disp, const float* gout, const void* keys, int F, int H, int W, const float* baselines6,
                    const float* trig, const double* xforms, const int32_t* adj_rowptr, const int32_t* adj_target,
                    const float* adj_weight, int n_adj, int flags, float* gdisp, float* gconf, mode_stream_t stream) {
  MODE_REQUIRE(F >= 0 && H > 0 && W > 0 && 3LL * F * H * W < (1LL << 31), MODE_ERR_BAD_ARG, "%s: bad size %d x %dx%d", who, F, H, W);
  MODE_REQUIRE((flags & ~(MODE_MV_CONF_PNG | MODE_MV_DEPTH_ONLY)) == 0, MODE_ERR_BAD_ARG, "%s: unknown flags 0x%x", who, flags);
  if (FULL) {
    MODE_REQUIRE(!(flags & MODE_MV_DEPTH_ONLY), MODE_ERR_BAD_ARG, "%s: MODE_MV_DEPTH_ONLY has no confidence channels", who);
    MODE_REQUIRE(!(flags & MODE_MV_CONF_PNG), MODE_ERR_BAD_ARG,
                 "%s: MODE_MV_CONF_PNG rounds the confidence to 8 bits, which is piecewise constant: it has no gradient", who);
  }
  MODE_REQUIRE(n_adj >= 0 && n_adj <= 8LL * H * W, MODE_ERR_BAD_ARG, "%s: %d adjoint entries for two %dx%d grids", who, n_adj, H, W);
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(disp && gout && baselines6 && trig && xforms && adj_rowptr && gdisp && (!FULL || gconf) &&
                   (n_adj == 0 || (adj_target && adj_weight)),
               MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(keys, MODE_ERR_WORKSPACE, "%s: the forward's key planes are required", who);
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(keys) & 7) == 0, MODE_ERR_WORKSPACE, "%s: unaligned key planes", who);
  MvArgs a;
  for (int p = 0; p < 6; ++p) a.baseline[p] = baselines6[p];
  for (int v = 0; v < 3; ++v) {
    for (int k = 0; k < 9; ++k) a.xf[v].R[k] = xforms[12 * v + k];
    for (int k = 0; k < 3; ++k) a.xf[v].t[k] = xforms[12 * v + 9 + k];
  }
  a.png = 0;  // (q is the identity wherever the confidence channels of gout are read)
  a.oc = (flags & MODE_MV_DEPTH_ONLY) ? 1 : 2;
  hipStream_t st = mode::as_stream(stream);
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(mv_bwd_sources_kernel<FULL>, dim3(grid_for(6LL * F * hw)), dim3(NT), 0, st, disp, gout, adj_rowptr, adj_target,
                     adj_weight, n_adj, gdisp, F, H, W, a, gconf);
  hipLaunchKernelGGL(mv_bwd_winners_kernel<FULL>, dim3(grid_for(3LL * F * hw)), dim3(NT), 0, st,
                     reinterpret_cast<const unsigned long long*>(keys), disp, gout, trig, gdisp, F, H, W, a, gconf);
  return mode::check_launch(who);
}

}  // namespace

extern "C" int mode_multiview_handoff_bwd(const float* disp, const float* gout, const void* keys, int F, int H, int W,
                                          const float* baselines6, const float* trig, const double* xforms, const int32_t* adj_rowptr,
                                          const int32_t* adj_target, const float* adj_weight, int n_adj, int flags, float* gdisp,
                                          mode_stream_t stream) {
  return handoff_bwd_run<false>("mode_multiview_handoff_bwd", disp, gout, keys, F, H, W, baselines6, trig, xforms, adj_rowptr, adj_target,
                                adj_weight, n_adj, flags, gdisp, nullptr, stream);
}

extern "C" int mode_multiview_handoff_bwd_full(const float* disp, const float* gout, const void* keys, int F, int H, int W,
                                               const float* baselines6, const float* trig, const double* xforms,
                                               const int32_t* adj_rowptr, const int32_t* adj_target, const float* adj_weight, int n_adj,
                                               int flags, float* gdisp, float* gconf, mode_stream_t stream) {
  return handoff_bwd_run<true>("mode_multiview_handoff_bwd_full", disp, gout, keys, F, H, W, baselines6, trig, xforms, adj_rowptr,
                               adj_target, adj_weight, n_adj, flags, gdisp, gconf, stream);
}
