// The multi-view hand-off for any camera rig: the contract of multiview.hip with 6 -> P.  The P pairs of a frame are of
// any kind (the sine rule alone; + rotateCassini; + depthViewTransWithConf) in any order, each with its own baseline and its own grid
// or view transform, and every plane has the bits the single-map entries give for its pair: the kernels here are new, the per-pixel
// arithmetic is that of geometry_internal.h and multiview_internal.h, shared with geometry.hip and multiview.hip.
//   launch 1  every key plane of the V view-transformed maps of every frame = +inf (mode::fill_words)     [V > 0]
//   launch 2  one thread per SOURCE pixel of the F x P disparity maps
//   launch 3  one thread per TARGET pixel of the F x V view-transformed maps                               [V > 0]
// The pair is uniform per workgroup: the grid is (blocks over a plane, P or V, frames), so kind, baseline and table index of the
// workgroup's pair -- and the 96 bytes of its view transform -- are read from the kernel arguments with scalar loads at an index that
// blockIdx.y alone decides, and the kind is a branch the whole workgroup takes the same way.  (multiview.hip indexes a.baseline[p] with a
// per-thread p; its argument structure is 0.3 KB.  Here it is 1.8 KB, which a per-thread index would copy to scratch.)
#include "common.h"
#include "geometry_internal.h"
#include "multiview_internal.h"

namespace {

namespace geom = mode::geom;
using namespace mode::mv;
constexpr int NT = 256;
constexpr int MAXP = MODE_MV_MAX_PAIRS;

struct RigArgs {
  float baseline[MAXP];  // per pair
  int kind[MAXP];        // per pair: MODE_MV_IDENTITY / ROTATE / VIEW
  int table[MAXP];       // per pair: its rotation grid, or its view transform and key plane
  int view_pair[MAXP];   // per view table index: the pair that names it
  int order_bwd[MAXP];   // the gradient's blockIdx.y -> pair, the rotated planes first: workgroups are dispatched in grid order, and the
                         // planes that cost an order of magnitude more than the others must not start last.  (The forward keeps the
                         // pair order: its view planes are bound by arithmetic and the others by memory, and with the view planes all
                         // dispatched first the two no longer overlap -- measured slower)
  int P, V;
  int png;               // MODE_MV_CONF_PNG
  int oc;                // output channels per pair: 2 (depth, confidence) or 1 (MODE_MV_DEPTH_ONLY)
};

struct RigXforms {
  geom::ViewXform xf[MAXP];  // per view table index
};

__device__ __forceinline__ float conf_out(const RigArgs& a, float c) { return a.png ? conf_png(c) : c; }

__global__ __launch_bounds__(NT) void rig_pairs_kernel(const float* __restrict__ disp, const float* __restrict__ conf,
                                                       const float* __restrict__ rot_grids, const float* __restrict__ trig,
                                                       unsigned long long* __restrict__ keys, float* __restrict__ out, int F, int H,
                                                       int W, RigArgs a, RigXforms x) {
  const long long hw = (long long)H * W;
  const int p = blockIdx.y;
  const int kind = a.kind[p], tab = a.table[p];
  const float baseline = a.baseline[p];
  for (int f = blockIdx.z; f < F; f += gridDim.z) {
    const long long plane = (long long)f * a.P + p;
    const float* dp = disp + plane * hw;
    const float* cp = conf + plane * hw;
    float* ob = out + plane * a.oc * hw;  // out[f, oc * p] (+ hw: out[f, 2p + 1])
    for (long long pix = (long long)blockIdx.x * NT + threadIdx.x; pix < hw; pix += (long long)gridDim.x * NT) {
      const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
      float* od = ob + pix;
      if (kind == MODE_MV_IDENTITY) {
        od[0] = geom::sine_rule_depth(dp[pix], j, W, baseline);
        if (a.oc == 2) od[hw] = conf_out(a, cp[pix]);
      } else if (kind == MODE_MV_ROTATE) {
        // rotateCassini on grid `tab` of (R, H, W, 2): the sampled source is the sine-rule depth of the same map
        const float2 g = reinterpret_cast<const float2*>(rot_grids)[tab * hw + pix];
        const geom::Bilinear b = geom::bilinear_border(g, H, W);
        od[0] = geom::bilinear_sum(b, [=](int y, int x) { return geom::sine_rule_depth(dp[(long long)y * W + x], x, W, baseline); });
        if (a.oc == 2) od[hw] = conf_out(a, geom::bilinear_sum(b, [=](int y, int x) { return cp[(long long)y * W + x]; }));
      } else {
        // depthViewTransWithConf: this source pixel's bid for its target in the key plane of (f, tab)
        const geom::ViewXform& xf = x.xf[tab];
        double r2;
        long long tgt;
        if (geom::project_pixel(geom::sine_rule_depth(dp[pix], j, W, baseline), trig[j], trig[W + j], trig[2 * W + i],
                                trig[2 * W + H + i], xf, H, W, r2, tgt))
          atomicMin(keys + ((long long)f * a.V + tab) * hw + tgt, geom::zkey(r2, pix, hw));
      }
    }
  }
}

__global__ __launch_bounds__(NT) void rig_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ conf,
                                                         float* __restrict__ out, int F, int H, int W, RigArgs a) {
  const long long hw = (long long)H * W;
  const int v = blockIdx.y;
  const int p = a.view_pair[v];
  for (int f = blockIdx.z; f < F; f += gridDim.z) {
    const long long plane = (long long)f * a.P + p;
    const unsigned long long* kp = keys + ((long long)f * a.V + v) * hw;
    float* ob = out + plane * a.oc * hw;
    for (long long pix = (long long)blockIdx.x * NT + threadIdx.x; pix < hw; pix += (long long)gridDim.x * NT) {
      const float2 vc = geom::resolve_key(kp[pix], conf + plane * hw, hw);
      ob[pix] = vc.x;
      if (a.oc == 2) ob[hw + pix] = conf_out(a, vc.y);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The gradient (mode_multiview_rig_handoff_bwd, and with FULL mode_multiview_rig_handoff_bwd_full), by the rules of multiview.hip:
//   launch A  one thread per SOURCE pixel of the F x P maps: identity and rotate planes get their value, view planes get +0
//   launch B  one thread per TARGET pixel of the F x V view-transformed maps: the winner of its key gets the target's gradient [V > 0]
// A source bids for one target, so it wins at most one: launch B's stores never collide, and no sum is formed with atomics.
template <bool FULL>
__global__ __launch_bounds__(NT) void rig_bwd_sources_kernel(const float* __restrict__ disp, const float* __restrict__ gout,
                                                             const int* __restrict__ rowptr, const int* __restrict__ target,
                                                             const float* __restrict__ weight, int n_adj, float* __restrict__ gdisp,
                                                             int F, int H, int W, RigArgs a, float* __restrict__ gconf) {
  const long long hw = (long long)H * W;
  const int p = a.order_bwd[blockIdx.y];
  const int kind = a.kind[p], tab = a.table[p];
  const float baseline = a.baseline[p];
  for (int f = blockIdx.z; f < F; f += gridDim.z) {
    const long long plane = (long long)f * a.P + p;
    const float* gd = gout + plane * a.oc * hw;  // gout[f, oc * p]; FULL (oc = 2): gd + hw = gout[f, 2p + 1]
    for (long long pix = (long long)blockIdx.x * NT + threadIdx.x; pix < hw; pix += (long long)gridDim.x * NT) {
      const long long idx = plane * hw + pix;
      float g = 0.f, gc = 0.f;  // view pairs: launch B fills the winners in
      if (kind != MODE_MV_VIEW) {
        const int j = (int)(pix % W);
        const float s = sine_rule_slope(disp[idx], j, W, baseline);
        if (kind == MODE_MV_IDENTITY) {
          if (s != 0.f) g = gd[pix] * s;
          if (FULL) gc = gd[hw + pix];
        } else if (FULL || s != 0.f) {
          // the (target, weight) entries of the rotation grid whose corner this source is, in the list's stored order
          const int* rp = rowptr + tab * (hw + 1) + pix;
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
}

template <bool FULL>
__global__ __launch_bounds__(NT) void rig_bwd_winners_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ disp,
                                                             const float* __restrict__ gout, const float* __restrict__ trig,
                                                             float* __restrict__ gdisp, int F, int H, int W, RigArgs a, RigXforms x,
                                                             float* __restrict__ gconf) {
#pragma clang fp contract(off)  // r2 as geom::project_pixel rounds it
  const long long hw = (long long)H * W;
  const int v3 = blockIdx.y;
  const int p = a.view_pair[v3];
  const float baseline = a.baseline[p];
  const geom::ViewXform& xf = x.xf[v3];
  for (int f = blockIdx.z; f < F; f += gridDim.z) {
    const long long plane = (long long)f * a.P + p;
    const unsigned long long* kp = keys + ((long long)f * a.V + v3) * hw;
    for (long long pix = (long long)blockIdx.x * NT + threadIdx.x; pix < hw; pix += (long long)gridDim.x * NT) {
      const unsigned long long k = kp[pix];
      if (k == ~0ull) continue;  // no source reached this target
      const float v = __uint_as_float((unsigned)(k >> 32));
      // geom::resolve_key: capped (strictly above; its 100000 -> 0 rule lies above the cap too): a constant depth.  Its confidence is
      // the winner's all the same, so FULL decodes the winner first.
      if (!FULL && v > 1000.f) continue;
      const unsigned lo = (unsigned)(k & 0xffffffffull);
      const long long src = (lo & 0x80000000u) ? (long long)(lo & 0x7fffffffu) : hw - 1 - (long long)lo;
      if (src < 0 || src >= hw) continue;  // (not a key of this size's forward)
      if (FULL) {
        gconf[plane * hw + src] = gout[(plane * 2 + 1) * hw + pix];
        if (v > 1000.f) continue;
      }
      const int i = (int)(src / W), j = (int)(src - (long long)i * W);
      const float d = disp[plane * hw + src];
      const float s = sine_rule_slope(d, j, W, baseline);
      if (s == 0.f) continue;
      // r2 = |r1 dir - t| (R is orthonormal), so d r2 / d r1 = (r1 - dir . t) / r2 with |dir| = 1
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
}

// blocks over one plane x pairs (or view pairs) x frames: about 8 workgroups per CU in all, and every thread has a pixel of its plane
dim3 grid_for(long long hw, int planes, int F) {
  const int fz = std::min(F, 65535);
  const long long want = std::max<long long>(1, 8LL * kNumCU / ((long long)planes * fz));
  return dim3((unsigned)std::min<long long>(mode::cdiv(hw, NT), want), (unsigned)planes, (unsigned)fz);
}

// The same for the gradient's pass over the sources, where every PLANE gets up to 8 workgroups per CU of its own: there the planes
// differ in cost by an order of magnitude (a rotated plane's adjoint-list walk against a copy or a zero), and with the chip's worth of
// workgroups divided among the planes the expensive ones run on a fraction of it while the cheap ones have finished.  The
// forward's planes are cheap and nearer to each other; there more workgroups are only more set-up.
dim3 grid_per_plane(long long hw, int planes, int F) {
  return dim3((unsigned)std::min<long long>(mode::cdiv(hw, NT), 8LL * kNumCU), (unsigned)planes, (unsigned)std::min(F, 65535));
}

// The checks that the three launching entries share, and the kernel arguments they fill in: the records, R and V, the transforms.
int rig_args(const char* who, int F, int P, int H, int W, const mode_mv_pair* pairs, int R, int V, const double* xforms, int flags,
             RigArgs& a, RigXforms& x) {
  MODE_REQUIRE(P >= 1 && P <= MAXP, MODE_ERR_BAD_ARG, "%s: %d pairs, not 1 .. %d", who, P, MAXP);
  // 2 P F H W < 2^31, formed so that no product can overflow whatever F, H and W are: H W < 2^62, 2 P H W < 2^36
  MODE_REQUIRE(F >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && F <= ((1LL << 31) - 1) / (2LL * P * ((long long)H * W)),
               MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %dx%d", who, F, P, H, W);
  MODE_REQUIRE((flags & ~(MODE_MV_CONF_PNG | MODE_MV_DEPTH_ONLY)) == 0, MODE_ERR_BAD_ARG, "%s: unknown flags 0x%x", who, flags);
  MODE_REQUIRE(pairs, MODE_ERR_BAD_ARG, "%s: null pointer (pairs)", who);
  MODE_REQUIRE(R >= 0 && V >= 0 && R <= P && V <= P, MODE_ERR_BAD_ARG, "%s: R = %d, V = %d for %d pairs", who, R, V, P);
  int nr = 0, nv = 0;
  unsigned seen_r = 0, seen_v = 0;
  a = RigArgs{};
  for (int p = 0; p < P; ++p) {
    const int kind = pairs[p].kind, tab = pairs[p].table;
    MODE_REQUIRE(kind == MODE_MV_IDENTITY || kind == MODE_MV_ROTATE || kind == MODE_MV_VIEW, MODE_ERR_BAD_ARG, "%s: pair %d has unknown kind %d",
                 who, p, kind);
    a.kind[p] = kind;
    a.baseline[p] = pairs[p].baseline;
    if (kind == MODE_MV_IDENTITY) continue;
    const int n = kind == MODE_MV_ROTATE ? R : V;
    unsigned& seen = kind == MODE_MV_ROTATE ? seen_r : seen_v;
    MODE_REQUIRE(tab >= 0 && tab < n, MODE_ERR_BAD_ARG, "%s: pair %d has table index %d, not 0 .. %d", who, p, tab, n - 1);
    MODE_REQUIRE(!(seen >> tab & 1u), MODE_ERR_BAD_ARG, "%s: pair %d names table index %d a second time", who, p, tab);
    seen |= 1u << tab;
    a.table[p] = tab;
    if (kind == MODE_MV_ROTATE) {
      ++nr;
    } else {
      ++nv;
      a.view_pair[tab] = p;
    }
  }
  MODE_REQUIRE(nr == R && nv == V, MODE_ERR_BAD_ARG, "%s: R = %d, V = %d, but the pairs hold %d rotations and %d view transforms", who, R, V,
               nr, nv);
  MODE_REQUIRE(V == 0 || xforms, MODE_ERR_BAD_ARG, "%s: null pointer (xforms)", who);
  a.P = P;
  a.V = V;
  int nb = 0;
  for (int kind : {MODE_MV_ROTATE, MODE_MV_IDENTITY, MODE_MV_VIEW})
    for (int p = 0; p < P; ++p)
      if (a.kind[p] == kind) a.order_bwd[nb++] = p;
  a.png = (flags & MODE_MV_CONF_PNG) ? 1 : 0;
  a.oc = (flags & MODE_MV_DEPTH_ONLY) ? 1 : 2;
  x = RigXforms{};
  for (int v = 0; v < V; ++v) {
    for (int k = 0; k < 9; ++k) x.xf[v].R[k] = xforms[12 * v + k];
    for (int k = 0; k < 3; ++k) x.xf[v].t[k] = xforms[12 * v + 9 + k];
  }
  return MODE_OK;
}

}  // namespace

extern "C" size_t mode_multiview_rig_handoff_workspace_bytes(int F, int V, int H, int W) {
  // 0 for sizes the launching entries refuse (2 V F H W >= 2^31 among them: V <= P), the bound formed without a product that can overflow
  if (!(F > 0 && V > 0 && V <= MAXP && H > 0 && W > 0)) return 0;
  const long long hw = (long long)H * W;
  if (hw >= (1LL << 31) || F > ((1LL << 31) - 1) / (2LL * V * hw)) return 0;
  return (size_t)V * F * hw * sizeof(unsigned long long);
}

extern "C" int mode_multiview_rig_handoff(const float* disp, const float* conf, int F, int P, int H, int W, const mode_mv_pair* pairs,
                                          int R, const float* rot_grids, const float* trig, int V, const double* xforms, int flags,
                                          float* out, void* workspace, mode_stream_t stream) {
  const char* who = "mode_multiview_rig_handoff";
  RigArgs a;
  RigXforms x;
  const int rc = rig_args(who, F, P, H, W, pairs, R, V, xforms, flags, a, x);
  if (rc != MODE_OK) return rc;
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(disp && conf && out && (R == 0 || rot_grids) && (V == 0 || trig), MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(rot_grids) & 7) == 0, MODE_ERR_BAD_ARG, "%s: rotation grids must be 8-byte aligned", who);
  MODE_REQUIRE(V == 0 || workspace, MODE_ERR_WORKSPACE, "%s: workspace required", who);
  MODE_REQUIRE(V == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MODE_ERR_WORKSPACE, "%s: unaligned workspace", who);
  hipStream_t st = mode::as_stream(stream);
  const long long hw = (long long)H * W;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
  if (V > 0) {
    // all keys = +inf (a kernel, not hipMemsetAsync: common.h)
    const int frc = mode::fill_words(workspace, 0xffffffffu, 2 * (size_t)V * F * hw, st, who);
    if (frc != MODE_OK) return frc;
  }
  hipLaunchKernelGGL(rig_pairs_kernel, grid_for(hw, P, F), dim3(NT), 0, st, disp, conf, rot_grids, trig, keys, out, F, H, W, a, x);
  if (V > 0) hipLaunchKernelGGL(rig_resolve_kernel, grid_for(hw, V, F), dim3(NT), 0, st, keys, conf, out, F, H, W, a);
  return mode::check_launch(who);
}

namespace {

// mode_multiview_rig_handoff_bwd (FULL = false, gconf unread) and mode_multiview_rig_handoff_bwd_full: the same checks and launches
template <bool FULL>
int rig_bwd_run(const char* who, const float* disp, const float* gout, const void* keys, int F, int P, int H, int W,
                const mode_mv_pair* pairs, int R, const float* trig, int V, const double* xforms, const int32_t* adj_rowptr,
                const int32_t* adj_target, const float* adj_weight, int n_adj, int flags, float* gdisp, float* gconf,
                mode_stream_t stream) {
  RigArgs a;
  RigXforms x;
  const int rc = rig_args(who, F, P, H, W, pairs, R, V, xforms, flags, a, x);
  if (rc != MODE_OK) return rc;
  if (FULL) {
    MODE_REQUIRE(!(flags & MODE_MV_DEPTH_ONLY), MODE_ERR_BAD_ARG, "%s: MODE_MV_DEPTH_ONLY has no confidence channels", who);
    MODE_REQUIRE(!(flags & MODE_MV_CONF_PNG), MODE_ERR_BAD_ARG,
                 "%s: MODE_MV_CONF_PNG rounds the confidence to 8 bits, which is piecewise constant: it has no gradient", who);
  }
  MODE_REQUIRE(n_adj >= 0 && n_adj <= 4LL * R * H * W, MODE_ERR_BAD_ARG, "%s: %d adjoint entries for %d %dx%d grids", who, n_adj, R, H, W);
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(disp && gout && gdisp && (!FULL || gconf) && (V == 0 || trig) && (R == 0 || adj_rowptr) &&
                   (n_adj == 0 || (adj_target && adj_weight)),
               MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(V == 0 || keys, MODE_ERR_WORKSPACE, "%s: the forward's key planes are required", who);
  MODE_REQUIRE(V == 0 || (reinterpret_cast<uintptr_t>(keys) & 7) == 0, MODE_ERR_WORKSPACE, "%s: unaligned key planes", who);
  a.png = 0;  // (q is the identity wherever the confidence channels of gout are read)
  hipStream_t st = mode::as_stream(stream);
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(rig_bwd_sources_kernel<FULL>, grid_per_plane(hw, P, F), dim3(NT), 0, st, disp, gout, adj_rowptr, adj_target, adj_weight,
                     n_adj, gdisp, F, H, W, a, gconf);
  if (V > 0)
    hipLaunchKernelGGL(rig_bwd_winners_kernel<FULL>, grid_for(hw, V, F), dim3(NT), 0, st,
                       reinterpret_cast<const unsigned long long*>(keys), disp, gout, trig, gdisp, F, H, W, a, x, gconf);
  return mode::check_launch(who);
}

}  // namespace

extern "C" int mode_multiview_rig_handoff_bwd(const float* disp, const float* gout, const void* keys, int F, int P, int H, int W,
                                              const mode_mv_pair* pairs, int R, const float* trig, int V, const double* xforms,
                                              const int32_t* adj_rowptr, const int32_t* adj_target, const float* adj_weight, int n_adj,
                                              int flags, float* gdisp, mode_stream_t stream) {
  return rig_bwd_run<false>("mode_multiview_rig_handoff_bwd", disp, gout, keys, F, P, H, W, pairs, R, trig, V, xforms, adj_rowptr,
                            adj_target, adj_weight, n_adj, flags, gdisp, nullptr, stream);
}

extern "C" int mode_multiview_rig_handoff_bwd_full(const float* disp, const float* gout, const void* keys, int F, int P, int H, int W,
                                                   const mode_mv_pair* pairs, int R, const float* trig, int V, const double* xforms,
                                                   const int32_t* adj_rowptr, const int32_t* adj_target, const float* adj_weight,
                                                   int n_adj, int flags, float* gdisp, float* gconf, mode_stream_t stream) {
  return rig_bwd_run<true>("mode_multiview_rig_handoff_bwd_full", disp, gout, keys, F, P, H, W, pairs, R, trig, V, xforms, adj_rowptr,
                           adj_target, adj_weight, n_adj, flags, gdisp, gconf, stream);
}
