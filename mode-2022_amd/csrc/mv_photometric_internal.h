// What the multi-view reprojection kernels share: mv_photometric.hip (the loss and its gradient to the depth)
// and mv_pose_grad.hip (its gradient to the sources' poses).  Every piece here was moved out of mv_photometric.hip unchanged, under
// the rule of photometric_internal.h: a kernel compiles to the same gfx950 code with a piece as it did with its own copy.  The pieces
// stay in an unnamed namespace, as they were: the kernels take Poses by value, so its name is part of theirs.
//
// Here: the poses as a kernel argument, the LDS planes of one tile and its halo, the viewing direction of a pixel, THE fp64 geometry
// (project), the bilinear sample, the two staging loops, and the checks that every launching entry of the family makes.
#pragma once
#include "mode_hip_mvphoto.h"
#include "photometric_internal.h"

static_assert(MODE_MVP_STATS == MODE_MVP_WINS + MODE_MVP_MAX_SOURCES, "one win count per source after the four sums");
static_assert(MODE_MVP_NO_WINNER >= MODE_MVP_MAX_SOURCES && MODE_MVP_NO_WINNER <= 255, "win is a byte");

namespace {

using namespace mode::photometric;

constexpr int PX = TH * TW / NT;  // tile pixels per thread
constexpr int kS = MODE_MVP_STATS;
constexpr int kMaxS = MODE_MVP_MAX_SOURCES;
constexpr int kNone = MODE_MVP_NO_WINNER;
constexpr double kPi = 3.14159265358979323846;

// Kernel-side copies of the parameters and of the poses (by value: they travel in the kernel arguments).
using Prm = Colour;

struct Poses {
  double p[kMaxS][12];  // [A | o], row-major 3 x 4
};

template <int HALO>
struct Stage {
  static constexpr int RH = TH + 2 * HALO, RW = TW + 2 * HALO, N = RH * RW;
  static constexpr int PER_THREAD = (N + NT - 1) / NT;
  float L[3][N];   // reference image, de-normalised
  float R[3][N];   // the current source warped to the reference view (0 where invalid)
  float ld[N];     // log depth (0 where the depth is not finite and > 0)
  unsigned char ok[N];   // valid for the current source
  unsigned char dok[N];  // depth finite and > 0
};

struct Dir {
  double x, y, z;
};

#ifdef __HIPCC__
// The viewing direction of pixel (h, w), angles at the pixel's centre.
__device__ __forceinline__ Dir pixel_dir(int h, int w, int H, int W) {
  const double theta = kPi - ((double)h + 0.5) * 2.0 * kPi / (double)H;
  const double phi = kPi / 2 - ((double)w + 0.5) * kPi / (double)W;
  double st, ct, sp, cp;
  sincos(theta, &st, &ct);
  sincos(phi, &sp, &cp);
  Dir n;
  n.x = sp;
  n.y = cp * st;
  n.z = cp * ct;
  return n;
}

// Where one pixel lands in one source and how that moves with its depth.
struct Geo {
  int x0, ya, yb;  // columns x0, x0 + 1 (0 <= x0 <= W - 2); rows ya = y0 mod H, yb = (y0 + 1) mod H
  float t, q;      // u - x0, v - y0
  float du, dv;    // du / dD, dv / dD (SLOPES only)
};

// THE geometry, fp64, for forward and backward alike: depth D along n, pose P = [A | o] -> whether the pixel is valid for the source
// and, if so, g.  Rounded to fp32 only at t, q, du, dv.
template <bool SLOPES>
__device__ __forceinline__ bool project(float depth, const Dir& n, const double* __restrict__ P, int H, int W, Geo& g) {
  if (!(__builtin_isfinite(depth) && depth > 0.f)) return false;
  const double D = (double)depth;
  const double mx = P[0] * n.x + P[1] * n.y + P[2] * n.z;
  const double my = P[4] * n.x + P[5] * n.y + P[6] * n.z;
  const double mz = P[8] * n.x + P[9] * n.y + P[10] * n.z;
  const double Yx = D * mx + P[3], Yy = D * my + P[7], Yz = D * mz + P[11];
  const double s2 = Yy * Yy + Yz * Yz;
  const double r2 = Yx * Yx + s2;
  const double rho = sqrt(r2);
  if (!(rho > 0.0)) return false;
  const double phi = asin(Yx / rho);
  const double theta = atan2(Yy, Yz);
  const double u = (kPi / 2 - phi) * (double)W / kPi - 0.5;
  const double v = (kPi - theta) * (double)H / (2.0 * kPi) - 0.5;
  if (!(u >= 0.0 && u <= (double)(W - 1)) || !(v == v)) return false;  // pole to pole; this keeps the source's poles out as well
  const double fu = floor(u), fv = floor(v);
  int x0 = (int)fu;
  x0 = x0 < W - 2 ? x0 : W - 2;
  const int y0 = (int)fv;  // -1 .. H - 1
  g.x0 = x0;
  g.ya = ((y0 % H) + H) % H;
  g.yb = g.ya + 1 == H ? 0 : g.ya + 1;
  g.t = (float)(u - (double)x0);
  g.q = (float)(v - fv);
  if (SLOPES) {
    const double Ym = Yx * mx + Yy * my + Yz * mz;
    const double dphi = (mx * r2 - Yx * Ym) / (r2 * sqrt(s2));
    const double dtheta = (my * Yz - mz * Yy) / s2;
    g.du = (float)(-((double)W / kPi) * dphi);
    g.dv = (float)(-((double)H / (2.0 * kPi)) * dtheta);
  }
  return true;
}

// The bilinear value of the de-normalised source at g, and (SLOPES) d Ih / dD.  img: the three planes of one source of one frame.
template <bool SLOPES>
__device__ __forceinline__ void sample(const float* __restrict__ img, int HW, int W, const Geo& g, const Prm& p, float ih[3], float slope[3]) {
  const int a = g.ya * W + g.x0, b = g.yb * W + g.x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pl = img + c * HW;
    const float r00 = pl[a] * p.std[c] + p.mean[c], r01 = pl[a + 1] * p.std[c] + p.mean[c];
    const float r10 = pl[b] * p.std[c] + p.mean[c], r11 = pl[b + 1] * p.std[c] + p.mean[c];
    const float top = (1.f - g.t) * r00 + g.t * r01, bot = (1.f - g.t) * r10 + g.t * r11;
    ih[c] = (1.f - g.q) * top + g.q * bot;
    if (SLOPES) slope[c] = ((1.f - g.q) * (r01 - r00) + g.q * (r11 - r10)) * g.du + (bot - top) * g.dv;
  }
}

// What does not depend on the source, for tile (h0, w0) and its halo: L, log depth and its validity into LDS; the viewing direction
// and the depth of this thread's staged pixels into registers (dep = NaN for the columns outside [0, W): invalid for every source).
// Rows wrap modulo H; columns outside [0, W) are invalid pixels with L = 0 (no window that exists contains them).
template <int HALO>
__device__ __forceinline__ void stage_ref(Stage<HALO>& s, const float* __restrict__ ref, const float* __restrict__ depth, int H, int W,
                                          int h0, int w0, const Prm& p, Dir (&n)[Stage<HALO>::PER_THREAD], float (&dep)[Stage<HALO>::PER_THREAD]) {
  using S = Stage<HALO>;
  const int HW = H * W;
#pragma unroll
  for (int k = 0; k < S::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    dep[k] = __builtin_nanf("");
    n[k].x = n[k].y = n[k].z = 0.0;
    if (i >= S::N) continue;
    const int r = i / S::RW, c = i - r * S::RW;
    int h = (h0 - HALO + r) % H;
    h = h < 0 ? h + H : h;
    const int w = w0 - HALO + c;
    float l[3] = {0.f, 0.f, 0.f};
    float ld = 0.f;
    bool dok = false;
    if (w >= 0 && w < W) {
      const int off = h * W + w;
      const float d = depth[off];
      dep[k] = d;
      dok = __builtin_isfinite(d) && d > 0.f;
      ld = dok ? logf(d) : 0.f;
      n[k] = pixel_dir(h, w, H, W);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) l[ch] = ref[ch * HW + off] * p.std[ch] + p.mean[ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.L[ch][i] = l[ch];
    s.ld[i] = ld;
    s.dok[i] = dok ? 1 : 0;
  }
}

// One source warped into the R planes.  img: the three planes of that source of this frame; P: its pose.  SLOPES: d Ih / dD of the
// tile's own pixels (not the halo's) into slope[ch][r * TW + c].
template <int HALO, bool SLOPES>
__device__ __forceinline__ void stage_src(Stage<HALO>& s, const float* __restrict__ img, const double* __restrict__ P, int H, int W,
                                          const Prm& p, const Dir (&n)[Stage<HALO>::PER_THREAD], const float (&dep)[Stage<HALO>::PER_THREAD],
                                          float (*slope)[TH * TW]) {
  using S = Stage<HALO>;
#pragma unroll
  for (int k = 0; k < S::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    if (i >= S::N) continue;
    Geo g;
    float ih[3] = {0.f, 0.f, 0.f}, sl[3] = {0.f, 0.f, 0.f};
    const bool ok = project<SLOPES>(dep[k], n[k], P, H, W, g);
    if (ok) sample<SLOPES>(img, H * W, W, g, p, ih, sl);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.R[ch][i] = ih[ch];
    s.ok[i] = ok ? 1 : 0;
    if (SLOPES) {
      const int r = i / S::RW - HALO, c = i % S::RW - HALO;
      if (r >= 0 && r < TH && c >= 0 && c < TW) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) slope[ch][r * TW + c] = sl[ch];
      }
    }
  }
}
#endif  // __HIPCC__

// The checks the launching entries share; fills p, the poses and the tiling.
int check_common(const char* who, const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                 const mode_photometric_params* params, Prm& p, Poses& ps, int& tiles_w, int& tiles) {
  MODE_REQUIRE(ref && src && depth && poses && params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(S >= 1 && S <= kMaxS, MODE_ERR_BAD_ARG, "%s: S = %d source views (1 .. %d)", who, S, kMaxS);
  MODE_REQUIRE(F >= 1, MODE_ERR_BAD_ARG, "%s: bad number of frames %d", who, F);
  int rc = check_tiling(who, H, W, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  for (int s = 0; s < kMaxS; ++s)
    for (int k = 0; k < 12; ++k) ps.p[s][k] = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* P = poses + 12 * s;
    for (int k = 0; k < 12; ++k) MODE_REQUIRE(std::isfinite(P[k]), MODE_ERR_BAD_ARG, "%s: pose %d, entry %d is not finite", who, s, k);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double dot = P[4 * a] * P[4 * b] + P[4 * a + 1] * P[4 * b + 1] + P[4 * a + 2] * P[4 * b + 2];
        MODE_REQUIRE(fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-9, MODE_ERR_BAD_ARG,
                     "%s: pose %d: A is not orthonormal to 1e-9 (row %d . row %d = %.17g)", who, s, a, b, dot);
      }
    for (int k = 0; k < 12; ++k) ps.p[s][k] = P[k];
  }
  // Offsets into the sources of one call (3 F S H W) and the workgroup index (F x tiles) are 32-bit quantities; bases are 64-bit.
  MODE_REQUIRE(3ll * F * S * H * W < (1ll << 31), MODE_ERR_UNSUPPORTED,
               "%s: sources of 3 x %d x %d x %d x %d elements: 32-bit indices need 3 F S H W < 2^31", who, F, S, H, W);
  load_colour(params, p);
  return MODE_OK;
}

}  // namespace
