// What the forward-splatting kernels share: mv_visibility.hip (the z-buffer visibility masks) and mv_render.hip
// (novel-view rendering).  Every piece here was moved out of mv_visibility.hip unchanged, under the rule of photometric_internal.h: a
// kernel compiles to the same gfx950 code with a piece as it did with its own copy.  The pieces stay in an unnamed namespace, as they
// were.
//
// Here: the empty key, where a reference pixel lands in another view and at what range (land), the grid of a flat launch and the
// rounding of a workspace part.
#pragma once
#include "mv_photometric_internal.h"

namespace {

constexpr unsigned long long kEmpty = ~0ull;

struct Landing {
  double rho;
  int at;  // y * W + x in the source's plane, or -1 where the pixel is invalid for the source
};

#ifdef __HIPCC__
// Where a pixel lands in one source and at what range.  Validity is project<>'s, the very function the loss calls; project<> keeps
// rho, u and v to itself, so Y, rho, u and v are formed again here by the same expressions in the same order (as mv_pose_grad.hip
// rebuilds Y).  The landing pixel is clamped into the plane whatever the two evaluations make of their last bit.
__device__ __forceinline__ Landing land(float depth, const Dir& n, const double* __restrict__ P, int H, int W) {
  Landing l;
  l.rho = 0.0;
  l.at = -1;
  Geo g;
  if (!project<false>(depth, n, P, H, W, g)) return l;
  const double D = (double)depth;
  const double mx = P[0] * n.x + P[1] * n.y + P[2] * n.z;
  const double my = P[4] * n.x + P[5] * n.y + P[6] * n.z;
  const double mz = P[8] * n.x + P[9] * n.y + P[10] * n.z;
  const double Yx = D * mx + P[3], Yy = D * my + P[7], Yz = D * mz + P[11];
  const double s2 = Yy * Yy + Yz * Yz;
  const double r2 = Yx * Yx + s2;
  const double rho = sqrt(r2);
  const double phi = asin(Yx / rho);
  const double theta = atan2(Yy, Yz);
  const double u = (kPi / 2 - phi) * (double)W / kPi - 0.5;
  const double v = (kPi - theta) * (double)H / (2.0 * kPi) - 0.5;
  int x = (int)floor(u + 0.5);
  x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
  int y = (int)floor(v + 0.5);  // 0 .. H
  y = ((y % H) + H) % H;
  l.rho = rho;
  l.at = y * W + x;
  return l;
}
#endif  // __HIPCC__

int grid_for(long long n) { return (int)std::min<long long>(mode::cdiv(n, NT), 8LL * kNumCU); }

// The parts of a workspace are each 16-byte aligned.
size_t part(size_t bytes) { return (bytes + 15) / 16 * 16; }

}  // namespace
