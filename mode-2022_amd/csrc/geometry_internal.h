// Per-pixel arithmetic of the export-stage geometry, shared by the single-map entries (geometry.hip) and the batched multi-view
// hand-off (multiview.hip; multiview_rig.hip for any camera rig).  Every helper here is a piece of one of geometry.hip's kernels moved out of it unchanged, so whatever
// includes this header computes the old entries' bits (DESIGN 12 records the instruction-stream comparison of the move).
// (One later addition, bilinear_border_exact / bilinear_sum_exact for erp_ingest.hip, is new arithmetic beside them; it changes none.)
// Contraction: the helpers carry no fp-contract pragma of their own except project_pixel's (which was there before); do not add one
// and build with no fast-math flag: the bilinear `v += s * w` sums are where a fused multiply-add could appear or disappear.
#pragma once
#include <hip/hip_runtime.h>

namespace mode {
namespace geom {

// ---------------------------------------------------------------------------------------------------------------------
// disparity -> depth by the sine rule (save_output_disparity_stage.py:118-135), float32 arithmetic like numpy's:
//   phi_l = float(start + j * (-step))   (np.arange in float64, then .astype(float32))
//   phi_r = disp * pi / W + phi_l        depth = baseline * sin(pi/2 - phi_r) / sin(phi_r - phi_l)
//   disp == 0 -> 1000 (masked, filled);  depth > 1000 -> 1000;  depth < 0 -> 0
// `j` is the column of the pixel.
__device__ __forceinline__ float sine_rule_depth(float d, int j, int W, float baseline) {
  const float pi_f = 3.14159265358979323846f, half_pi_f = 1.57079632679489661923f;
  const double start = 0.5 * 3.14159265358979323846 - (0.5 * 3.14159265358979323846 / W);
  const double step = 3.14159265358979323846 / W;
  float out = 1000.f;
  if (d != 0.f) {
    const float phi_l = (float)(start + (double)j * (-step));
    const float phi_r = d * pi_f / (float)W + phi_l;
    out = baseline * sinf(half_pi_f - phi_r) / sinf(phi_r - phi_l);
    if (out > 1000.f) out = 1000.f;
    if (out < 0.f) out = 0.f;  // NaN stays NaN, as in numpy
  }
  return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// The bilinear tap of F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True) at normalised grid point g of a
// (Hs, Ws) source: the four corners and their weights.
struct Bilinear {
  int x0, y0, x1, y1;
  float nw, ne, sw, se;
  bool x1ok, y1ok;
};

__device__ __forceinline__ Bilinear bilinear_border(float2 g, int Hs, int Ws) {
  // unnormalise (align_corners=True), clip to the border
  float x = (g.x + 1.f) * 0.5f * (float)(Ws - 1);
  float y = (g.y + 1.f) * 0.5f * (float)(Hs - 1);
  x = fminf(fmaxf(x, 0.f), (float)(Ws - 1));
  y = fminf(fmaxf(y, 0.f), (float)(Hs - 1));
  const float xf = floorf(x), yf = floorf(y);
  const int x0 = (int)xf, y0 = (int)yf;
  const int x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = x - xf, wy1 = y - yf;
  const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  // corner weights in torch's order (nw, ne, sw, se); corners outside contribute nothing
  const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
  const bool x1ok = x1 <= Ws - 1, y1ok = y1 <= Hs - 1;
  return Bilinear{x0, y0, x1, y1, nw, ne, sw, se, x1ok, y1ok};
}

// The weighted sum over the corners, in torch's order; at(y, x) gives the source value of a corner (only corners inside are asked).
template <class At>
__device__ __forceinline__ float bilinear_sum(const Bilinear& b, At at) {
  float v = at(b.y0, b.x0) * b.nw;
  if (b.x1ok) v += at(b.y0, b.x1) * b.ne;
  if (b.y1ok) v += at(b.y1, b.x0) * b.sw;
  if (b.x1ok && b.y1ok) v += at(b.y1, b.x1) * b.se;
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same tap with the BITS of ATen's CPU kernel (GridSamplerKernel.cpp, the vectorised path torch 2.x takes for contiguous fp32
// input), for results that are truncated to bytes afterwards (erp_ingest.hip).  It differs from bilinear_border in the
// unnormalisation -- (g + 1) * ((size - 1) / 2), the scale formed first -- and from bilinear_sum in the sum, one fused multiply-add
// per corner after the first product, corners in the order nw, ne, sw, se:
//   v = fma(p_se, se, fma(p_sw, sw, fma(p_ne, ne, p_nw * nw)))
// Every operation goes through one of the helpers below, so neither the compiler's contraction nor a build flag can change it.
// HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators compiled under the header's own contraction setting: inlined next to each
// other the backend may still fuse them.  These carry `contract(off)` themselves (an instruction without the contract flag is never
// fused, whatever its neighbour allows); __fmaf_rn is a genuine fused multiply-add.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fmul_rn(a, b);
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fadd_rn(a, b);
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fsub_rn(a, b);
}

__device__ __forceinline__ Bilinear bilinear_border_exact(float2 g, int Hs, int Ws) {
  const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
  float x = mul_rn(add_rn(g.x, 1.f), mul_rn(xmax, 0.5f));  // ((size - 1) / 2 is exact in fp32 below 2^24)
  float y = mul_rn(add_rn(g.y, 1.f), mul_rn(ymax, 0.5f));
  x = fminf(fmaxf(x, 0.f), xmax);
  y = fminf(fmaxf(y, 0.f), ymax);
  const float xf = floorf(x), yf = floorf(y);
  const int x0 = (int)xf, y0 = (int)yf;
  const float ex = sub_rn(x, xf), ey = sub_rn(y, yf);
  const float wx = sub_rn(1.f, ex), wy = sub_rn(1.f, ey);
  return Bilinear{x0, y0, x0 + 1, y0 + 1, mul_rn(wx, wy), mul_rn(ex, wy), mul_rn(wx, ey), mul_rn(ex, ey), x0 + 1 < Ws, y0 + 1 < Hs};
}

// The sum over four corner VALUES (a corner outside the image is passed as 0, as ATen's masked gather returns it; its weight is 0).
__device__ __forceinline__ float bilinear_sum_exact(const Bilinear& b, float p_nw, float p_ne, float p_sw, float p_se) {
  return __fmaf_rn(p_se, b.se, __fmaf_rn(p_sw, b.sw, __fmaf_rn(p_ne, b.ne, mul_rn(p_nw, b.nw))));
}

// ---------------------------------------------------------------------------------------------------------------------
// depthViewTransWithConf.  Pass 1, one thread per SOURCE pixel (i, j) with r1 > 0:
//   X1 = r1 * dir(i, j)  (float32 products in numpy's order)  X2 = R (X1 - t)  (float64)       r2 = |X2|
//   I = clip(rint(H/2 - H * atan2(X2.y, X2.z) / (2 pi)), 0, H-1)      J = clip(rint(W/2 - W * asin(clip(X2.x / r2)) / pi), 0, W-1)
// and a 64-bit atomic min of a key into key[I][J].
// The reference scans the sources in row-major order and overwrites the target when r2 < view2[target] -- r2 in float64 against
// the float32 value stored so far (initial value 100000).  Let m be the smallest float32(r2) over the sources of a target
// (positive floats order like their bit patterns) and S the sources that round to m.  The first source of S always gets
// stored (rounding is monotonic); a later source of S replaces it only if its float64 r2 is strictly below the float32 m.
// Hence the survivor is the LAST source of L = {k in S : r2_k < m}, or the FIRST source of S when L is empty, and
//   key = bits(m) << 32 | (k in L ? 0 : 1) << 31 | (k in L ? N-1-k : k)
// has exactly that source as its minimum -- bit-identical to the sequential loop, in any execution order.
// Pass 2, one thread per TARGET pixel: view2 = r2 of the winner (0 if none; capped at 1000), conf2 = conf1[winner] (0 if none).
struct ViewXform {
  double R[9];
  double t[3];
};

// projection of one source pixel: returns false if it takes no part (r1 <= 0, r2 not below the initial 100000, r2 == 0)
__device__ __forceinline__ bool project_pixel(float r1, float sin_phi, float cos_phi, float sin_theta, float cos_theta,
                                              const ViewXform& xf, int H, int W, double& r2, long long& tgt) {
#pragma clang fp contract(off)  // numpy's matmul / sum of squares round every product: no fused multiply-adds here
  const double PI = 3.14159265358979323846;
  if (!(r1 > 0.f)) return false;
  // float32 products in numpy's order (geometry.py:126-128): r * sin(phi);  (r * cos(phi)) * sin(theta);  (r * cos(phi)) * cos(theta)
  const float rc = r1 * cos_phi;
  const float x1 = r1 * sin_phi, y1 = rc * sin_theta, z1 = rc * cos_theta;
  const double ax = (double)x1 - xf.t[0], ay = (double)y1 - xf.t[1], az = (double)z1 - xf.t[2];
  const double X = xf.R[0] * ax + xf.R[1] * ay + xf.R[2] * az;
  const double Y = xf.R[3] * ax + xf.R[4] * ay + xf.R[5] * az;
  const double Z = xf.R[6] * ax + xf.R[7] * ay + xf.R[8] * az;
  r2 = sqrt(X * X + Y * Y + Z * Z);
  if (!(r2 < 100000.0)) return false;  // never below the initial value (also drops NaN)
  const double theta = atan2(Y, Z);
  double sphi = X / r2;
  sphi = sphi < -1.0 ? -1.0 : (sphi > 1.0 ? 1.0 : sphi);
  const double phi = asin(sphi);
  double fi = rint((double)H / 2 - (double)H * theta / (2 * PI));
  double fj = rint((double)W / 2 - (double)W * phi / PI);
  fi = fi < 0.0 ? 0.0 : (fi > (double)(H - 1) ? (double)(H - 1) : fi);
  fj = fj < 0.0 ? 0.0 : (fj > (double)(W - 1) ? (double)(W - 1) : fj);
  if (!(fi == fi) || !(fj == fj)) return false;  // r2 == 0: NaN angles; numpy's int16 cast of NaN is platform noise
  tgt = (long long)fi * W + (long long)fj;
  return true;
}

// z-buffer key of source `idx` (of n) with radius r2, see above
__device__ __forceinline__ unsigned long long zkey(double r2, long long idx, long long n) {
  const float m = (float)r2;
  const bool inL = r2 < (double)m;
  const unsigned lo = inL ? (unsigned)(n - 1 - idx) : (0x80000000u | (unsigned)idx);
  return ((unsigned long long)__float_as_uint(m) << 32) | lo;
}

// pass 2 for one target pixel: its key k -> (view2, conf2), with conf1 the source plane of n pixels
__device__ __forceinline__ float2 resolve_key(unsigned long long k, const float* conf1, long long n) {
  float v = 0.f, c = 0.f;
  if (k != ~0ull) {
    v = __uint_as_float((unsigned)(k >> 32));
    const unsigned lo = (unsigned)(k & 0xffffffffull);
    c = conf1[(lo & 0x80000000u) ? (long long)(lo & 0x7fffffffu) : n - 1 - (long long)lo];
    if (v == 100000.f) v = 0.f;  // "view_2[view_2 == 100000] = 0"
    if (v > 1000.f) v = 1000.f;
  }
  return make_float2(v, c);
}

}  // namespace geom
}  // namespace mode
