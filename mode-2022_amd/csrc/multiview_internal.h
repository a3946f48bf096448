// Per-pixel arithmetic that the two hand-off translation units share: multiview.hip (the six pairs of a Deep360 frame) and
// multiview_rig.hip (the P pairs of any rig).  Each helper is a piece of multiview.hip moved out of it unchanged, so both files compute
// the same bits from one definition.  As in geometry_internal.h: no fp-contract pragma here and no fast-math flag in the build.
#pragma once
#include <hip/hip_runtime.h>

namespace mode {
namespace mv {

// The reference writes the confidence as an 8-bit PNG (cv2.imwrite(conf * 255): float32 product, saturate_cast<uchar> = round half
// to even and clamp) and reads it back as / 255.0 in float64, cast to float32 by the fusion loader.  NaN reads back as 0.
__device__ __forceinline__ float conf_png(float c) {
  const float r = fminf(255.f, fmaxf(0.f, rintf(c * 255.0f)));
  return (float)((double)r / 255.0);
}

// the sine rule without its clip, operation for operation as geom::sine_rule_depth forms it (d != 0)
__device__ __forceinline__ float sine_rule_raw(float d, int j, int W, float baseline, float& phi_l) {
  const float pi_f = 3.14159265358979323846f, half_pi_f = 1.57079632679489661923f;
  const double start = 0.5 * 3.14159265358979323846 - (0.5 * 3.14159265358979323846 / W);
  const double step = 3.14159265358979323846 / W;
  phi_l = (float)(start + (double)j * (-step));
  const float phi_r = d * pi_f / (float)W + phi_l;
  return baseline * sinf(half_pi_f - phi_r) / sinf(phi_r - phi_l);
}

// S(d, j) = d depth / d disparity = -(pi / W) baseline cos(phi_l) / sin^2(d pi / W) where the sine rule passes a gradient: d != 0 and
// 0 <= raw <= 1000 (the reference clips by assigning to the values strictly outside, so the boundary passes); exactly +0 elsewhere
// (NaN included).  The closed form has none of the forward's phi_r - phi_l cancellation.
__device__ __forceinline__ float sine_rule_slope(float d, int j, int W, float baseline) {
  if (d == 0.f) return 0.f;
  float phi_l;
  const float raw = sine_rule_raw(d, j, W, baseline, phi_l);
  if (!(raw >= 0.f && raw <= 1000.f)) return 0.f;
  const float pi_f = 3.14159265358979323846f;
  const float s = sinf(d * pi_f / (float)W);
  return -(pi_f / (float)W) * baseline * cosf(phi_l) / (s * s);
}

}  // namespace mv
}  // namespace mode
