// 3D60 ingest: what the reference's Dataset3D60Disparity.__getitem__ (dataloader/dataset3D60Loader.py:123-248) does on the
// host between the decoded equirectangular (ERP) files and ModeDisparity, for a whole batch.  See include/mode_hip.h.
//   mode_erp_pairs_u8_cassini  erp2rect_cassini of both RGB panoramas of every pair (utils/geometry.py:159-200: F.grid_sample, bilinear,
//                              border, align_corners) -> .astype(np.uint8) -> the stage-1 transform as a table lookup, and the mirrored
//                              twin (:193)
//   mode_erp_depth_disp        erp2rect_cassini of a depth map, the maxDepth threshold (:195-196) and __depth2disp (:258-270)
// The re-projection has the bits of ATen's CPU kernel (geom::bilinear_border_exact / bilinear_sum_exact): the bytes are a truncation of
// it, and a sum that is merely close turns 255 into 254 (or back) on every saturated region.
// A thread owns four consecutive pixels of a Cassini row: the grid points and the four weights of each are formed once and serve the
// left and the right image, their three channels and -- when all samples share one grid (G == 1) -- every sample the thread walks.
#include "common.h"
#include "geometry_internal.h"

namespace {

using mode::geom::Bilinear;
using mode::geom::bilinear_border_exact;
using mode::geom::bilinear_sum_exact;
using mode::geom::mul_rn;

constexpr int NT = 256;
constexpr int kLut = 256 * 3;  // lut[v * 3 + c], the table of ingest.hip

struct Quad {
  Bilinear b[4];
};

// the taps of pixels 4 q .. 4 q + 3 of grid plane `gp` ((H W, 2) fp32, 16-byte aligned; W % 4 == 0)
__device__ __forceinline__ Quad load_taps(const float* __restrict__ gp, long long q, int He, int We) {
  const float4 a = reinterpret_cast<const float4*>(gp)[2 * q], c = reinterpret_cast<const float4*>(gp)[2 * q + 1];
  Quad t;
  t.b[0] = bilinear_border_exact(make_float2(a.x, a.y), He, We);
  t.b[1] = bilinear_border_exact(make_float2(a.z, a.w), He, We);
  t.b[2] = bilinear_border_exact(make_float2(c.x, c.y), He, We);
  t.b[3] = bilinear_border_exact(make_float2(c.z, c.w), He, We);
  return t;
}

// trunc(bilinear) of the three channels of one pixel of an interleaved 8-bit image: r | g << 8 | b << 16
__device__ __forceinline__ unsigned sample_rgb(const unsigned char* __restrict__ img, const Bilinear& b, int We) {
  const unsigned char* nw = img + ((long long)b.y0 * We + b.x0) * 3;
  const unsigned char* sw = nw + (b.y1ok ? 3LL * We : 0);  // a corner outside is not read: the pointer stays on a valid pixel
  const int dx = b.x1ok ? 3 : 0;
  const bool seok = b.x1ok && b.y1ok;
  unsigned out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p_nw = (float)nw[c];
    const float p_ne = b.x1ok ? (float)nw[dx + c] : 0.f;
    const float p_sw = b.y1ok ? (float)sw[c] : 0.f;
    const float p_se = seok ? (float)sw[dx + c] : 0.f;
    const float v = bilinear_sum_exact(b, p_nw, p_ne, p_sw, p_se);
    out |= min((unsigned)v, 255u) << (8 * c);  // .astype(np.uint8) of a value in [0, 255]: truncation
  }
  return out;
}

__device__ __forceinline__ void store_planes(float* __restrict__ d, long long hw, const unsigned* px, const float* s_lut, bool reversed) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v0 = s_lut[3 * ((px[0] >> (8 * c)) & 255u) + c], v1 = s_lut[3 * ((px[1] >> (8 * c)) & 255u) + c];
    const float v2 = s_lut[3 * ((px[2] >> (8 * c)) & 255u) + c], v3 = s_lut[3 * ((px[3] >> (8 * c)) & 255u) + c];
    *reinterpret_cast<float4*>(d + c * hw) = reversed ? make_float4(v3, v2, v1, v0) : make_float4(v0, v1, v2, v3);
  }
}

// blockIdx.x: quads of one (H, W) plane; blockIdx.y: samples n = blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(NT) void erp_pairs_kernel(const unsigned char* __restrict__ pairs, const float* __restrict__ grid,
                                                       const float* __restrict__ lut, int N, int He, int We, int H, int W, int G,
                                                       float* __restrict__ left, float* __restrict__ right, float* __restrict__ left_flip,
                                                       float* __restrict__ right_flip, unsigned* __restrict__ cassini) {
  __shared__ float s_lut[kLut];
  for (int i = threadIdx.x; i < kLut; i += NT) s_lut[i] = lut[i];
  __syncthreads();
  const long long hw = (long long)H * W, ehw3 = 3LL * He * We;
  const int qpr = W / 4;
  const long long q = (long long)blockIdx.x * NT + threadIdx.x;
  if (q >= hw / 4) return;
  const int y = (int)(q / qpr), x = 4 * (int)(q - (long long)y * qpr);
  const long long at = (long long)y * W + x, at_flip = (long long)y * W + (W - 4 - x);
  Quad t;
  if (G == 1) t = load_taps(grid, q, He, We);
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    if (G != 1) t = load_taps(grid + 2 * hw * n, q, He, We);
    unsigned pl[4], pr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pl[k] = sample_rgb(pairs + (2LL * n) * ehw3, t.b[k], We);
      pr[k] = sample_rgb(pairs + (2LL * n + 1) * ehw3, t.b[k], We);
    }
    store_planes(left + 3 * hw * n + at, hw, pl, s_lut, false);
    store_planes(right + 3 * hw * n + at, hw, pr, s_lut, false);
    if (left_flip) {  // (both or neither: checked by the entry)
      store_planes(left_flip + 3 * hw * n + at_flip, hw, pr, s_lut, true);
      store_planes(right_flip + 3 * hw * n + at_flip, hw, pl, s_lut, true);
    }
    if (cassini) {  // 12 bytes per image: three dwords at a multiple of 12 bytes
      unsigned* cl = cassini + ((2LL * n) * hw + at) * 3 / 4;
      unsigned* cr = cassini + ((2LL * n + 1) * hw + at) * 3 / 4;
      cl[0] = pl[0] | (pl[1] << 24);
      cl[1] = (pl[1] >> 8) | (pl[2] << 16);
      cl[2] = (pl[2] >> 16) | (pl[3] << 8);
      cr[0] = pr[0] | (pr[1] << 24);
      cr[1] = (pr[1] >> 8) | (pr[2] << 16);
      cr[2] = (pr[2] >> 16) | (pr[3] << 8);
    }
  }
}

__device__ __forceinline__ float sample_f32(const float* __restrict__ img, const Bilinear& b, int We) {
  const float* nw = img + (long long)b.y0 * We + b.x0;
  const float* sw = nw + (b.y1ok ? We : 0);
  const int dx = b.x1ok ? 1 : 0;
  const float p_nw = nw[0];
  const float p_ne = b.x1ok ? nw[dx] : 0.f;
  const float p_sw = b.y1ok ? sw[0] : 0.f;
  const float p_se = (b.x1ok && b.y1ok) ? sw[dx] : 0.f;
  return bilinear_sum_exact(b, p_nw, p_ne, p_sw, p_se);
}

// __depth2disp on one pixel in numpy's order of operations and numpy 2's types; phi, s = sin(phi), c = cos(phi + pi / 2) of the OUTPUT
// column, float32 as numpy rounds them.  The reference's masked array is float32 while it meets arrays (d * sin(phi), d * d: float32
// products) and becomes float64 where it meets a Python scalar (+ baseline, 2 * d, ...), so everything from there on is float64; the
// result is rounded to float32 once, on the store.  (numpy 1 stayed in float32 throughout; near asin(1) -- depths far below the
// baseline -- that evaluation is up to 9.7e-4 px from this one on the fixtures, no margin under the 1e-3 px parity bound, which is
// why the wider type is the one kept: DESIGN 15.)
__device__ __forceinline__ float depth2disp(float d, float phi, float s, float c, double b, double Wd) {
#pragma clang fp contract(off)
  if (d <= 0.f) return __builtin_nanf("");  // the masked pixels: disp.filled(np.nan)  (d > maxDepth was zeroed before)
  const double num = (double)mul_rn(d, s) + b;
  const double den = ((double)mul_rn(d, d) + b * b) - ((2.0 * (double)d) * b) * (double)c;
  double r = num / sqrt(den);
  r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);  // np.clip: NaN stays NaN
  const double disp = Wd * (asin(r) - (double)phi) / 3.14159265358979323846;
  return (float)(disp < 0.0 ? 0.0 : disp);
}

__global__ __launch_bounds__(NT) void erp_depth_disp_kernel(const float* __restrict__ depth, const float* __restrict__ grid,
                                                            const float* __restrict__ cols, int N, int He, int We, int H, int W, int G,
                                                            double baseline, float maxdepth, int mirror, float* __restrict__ disp,
                                                            float* __restrict__ depth_cassini) {
  const long long hw = (long long)H * W, ehw = (long long)He * We;
  const int qpr = W / 4;
  const long long q = (long long)blockIdx.x * NT + threadIdx.x;
  if (q >= hw / 4) return;
  const int y = (int)(q / qpr), x = 4 * (int)(q - (long long)y * qpr);
  const int xo = mirror ? W - 4 - x : x;  // where the quad goes
  const long long at = (long long)y * W + xo;
  const float4 phi = *reinterpret_cast<const float4*>(cols + xo), s = *reinterpret_cast<const float4*>(cols + W + xo),
               c = *reinterpret_cast<const float4*>(cols + 2 * W + xo);
  const double Wd = (double)W;
  Quad t;
  if (G == 1) t = load_taps(grid, q, He, We);
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    if (G != 1) t = load_taps(grid + 2 * hw * n, q, He, We);
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = sample_f32(depth + ehw * n, t.b[k], We);
      d[k] = v > maxdepth ? 0.f : v;
    }
    const float4 dq = mirror ? make_float4(d[3], d[2], d[1], d[0]) : make_float4(d[0], d[1], d[2], d[3]);
    if (depth_cassini) *reinterpret_cast<float4*>(depth_cassini + hw * n + at) = dq;
    *reinterpret_cast<float4*>(disp + hw * n + at) =
        make_float4(depth2disp(dq.x, phi.x, s.x, c.x, baseline, Wd), depth2disp(dq.y, phi.y, s.y, c.y, baseline, Wd),
                    depth2disp(dq.z, phi.z, s.z, c.z, baseline, Wd), depth2disp(dq.w, phi.w, s.w, c.w, baseline, Wd));
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// n * H * W * per < 2^31 without forming a product that could overflow (n >= 0, H, W, per > 0)
bool fits31(long long n, int H, int W, int per) {
  const long long lim = (1LL << 31) - 1, hw = (long long)H * W;
  return hw <= lim / per && n <= lim / per / hw;
}

// sizes both entries share; `in_per` / `out_per`: elements per ERP / Cassini pixel of a sample
int check_sizes(const char* who, int N, int He, int We, int H, int W, int G, int in_per, int out_per) {
  MODE_REQUIRE(N >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size N = %d, Cassini %d x %d", who, N, H, W);
  MODE_REQUIRE(He >= 2 && We >= 2, MODE_ERR_BAD_ARG, "%s: bad ERP size %d x %d (both must be >= 2)", who, He, We);
  MODE_REQUIRE(W % 4 == 0, MODE_ERR_BAD_ARG, "%s: W = %d is not a multiple of 4", who, W);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(G == 1 || G == N, MODE_ERR_BAD_ARG, "%s: G = %d grids for N = %d samples (must be 1 or N)", who, G, N);
  MODE_REQUIRE(fits31(N, He, We, in_per) && fits31(N, H, W, out_per) && fits31(G, H, W, 2), MODE_ERR_BAD_ARG,
               "%s: bad size N = %d, ERP %d x %d, Cassini %d x %d (too large: an element count >= 2^31)", who, N, He, We, H, W);
  return MODE_OK;
}

// blocks over the quads of a plane x a split of the samples that fills the chip
dim3 launch_grid(int N, int H, int W) {
  const long long bx = mode::cdiv((long long)H * W / 4, NT);
  const long long by = std::min<long long>(N, std::max<long long>(1, (4LL * kNumCU + bx - 1) / bx));
  return dim3((unsigned)bx, (unsigned)by);
}

}  // namespace

extern "C" int mode_erp_pairs_u8_cassini(const uint8_t* pairs_u8, const float* grid, const float* lut, int N, int He, int We, int H, int W,
                                         int G, float* left, float* right, float* left_flip, float* right_flip, uint8_t* cassini_u8,
                                         mode_stream_t stream) {
  const char* who = "mode_erp_pairs_u8_cassini";
  if (int rc = check_sizes(who, N, He, We, H, W, G, 6, 6)) return rc;
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(pairs_u8 && grid && lut && left && right, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE((left_flip == nullptr) == (right_flip == nullptr), MODE_ERR_BAD_ARG, "%s: left_flip and right_flip go together (both or neither)",
               who);
  MODE_REQUIRE(aligned(grid, 16) && aligned(lut, 4), MODE_ERR_BAD_ARG, "%s: grid must be 16-byte aligned, lut 4-byte aligned", who);
  MODE_REQUIRE(aligned(left, 16) && aligned(right, 16) && aligned(left_flip, 16) && aligned(right_flip, 16) && aligned(cassini_u8, 4),
               MODE_ERR_BAD_ARG, "%s: float outputs must be 16-byte aligned, cassini_u8 4-byte aligned", who);
  hipLaunchKernelGGL(erp_pairs_kernel, launch_grid(N, H, W), dim3(NT), 0, mode::as_stream(stream), pairs_u8, grid, lut, N, He, We, H, W, G,
                     left, right, left_flip, right_flip, reinterpret_cast<unsigned*>(cassini_u8));
  return mode::check_launch(who);
}

extern "C" int mode_erp_depth_disp(const float* depth_erp, const float* grid, const float* cols, int N, int He, int We, int H, int W, int G,
                                   float baseline, float maxdepth, int mirror, float* disp, float* depth_cassini, mode_stream_t stream) {
  const char* who = "mode_erp_depth_disp";
  if (int rc = check_sizes(who, N, He, We, H, W, G, 1, 1)) return rc;
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(depth_erp && grid && cols && disp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(aligned(depth_erp, 4) && aligned(grid, 16) && aligned(cols, 16), MODE_ERR_BAD_ARG,
               "%s: grid and cols must be 16-byte aligned, depth_erp 4-byte aligned", who);
  MODE_REQUIRE(aligned(disp, 16) && aligned(depth_cassini, 16), MODE_ERR_BAD_ARG, "%s: outputs must be 16-byte aligned", who);
  // the float widened as it is: 0.26f is 3.7e-8 (relative) below the reference's double 0.26, at most 2e-6 px in a disparity
  const double b = (double)baseline;
  hipLaunchKernelGGL(erp_depth_disp_kernel, launch_grid(N, H, W), dim3(NT), 0, mode::as_stream(stream), depth_erp, grid, cols, N, He, We, H, W,
                     G, b, maxdepth, mirror ? 1 : 0, disp, depth_cassini);
  return mode::check_launch(who);
}
