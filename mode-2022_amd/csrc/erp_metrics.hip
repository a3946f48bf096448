// Scoring of fused depth in the equirectangular (ERP) domain (reference: test_fusion.py:76-100): see include/mode_hip.h.
//
// mode_erp_depth_metrics resamples prediction and ground truth of F Cassini frames to the ERP panorama, selects gt_erp <= maxdepth and
// reduces the statistics of mode_masked_metrics per frame, in one streaming pass and one fold launch.  The sampling arithmetic is
// geometry_internal.h's (the device functions of grid_sample_border_kernel), the reduction metrics_internal.h's, laid out so that
// row f has the bits of mode_masked_metrics on frame f's materialised ERP maps: blockIdx.y is the frame, gridDim.x =
// metric_blocks(H * W), quad q of ERP pixels (row-major ERP order) belongs to thread q % (gridDim.x * 256) and quads are walked
// ascending; frame f's slab is workspace + f * gridDim.x * MODE_METRICS_COUNT, folded by block f of the second launch.  No atomics:
// a row depends on its frame alone.
// mode_bicubic_up2 is the optional x2 upsampling in front of it (test_fusion.py:82).
#include "geometry_internal.h"
#include "metrics_internal.h"

namespace {

using namespace mode::metrics;
namespace geom = mode::geom;

template <bool kStore>
__global__ __launch_bounds__(NT) void erp_metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const float2* __restrict__ grid, int H, int W, float maxdepth,
                                                                 Thresholds th, double* __restrict__ slab,
                                                                 float* __restrict__ pred_erp, float* __restrict__ gt_erp) {
  __shared__ double sh[NT / 64][kS];
  Acc a = {};
  const int n = H * W;  // pixels of a frame, Cassini (H, W) or ERP (W, H)
  const int quads = (n + 3) / 4;
  const int stride = gridDim.x * NT;
  const long long base = (long long)blockIdx.y * n;
  const float* __restrict__ ps = pred + base;
  const float* __restrict__ gs = gt + base;
  for (int q = blockIdx.x * NT + threadIdx.x; q < quads; q += stride) {
    const int i0 = 4 * q;
    float p[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k < n ? i0 + k : n - 1;  // the n % 4 tail repeats the last pixel (never accumulated or stored)
      const geom::Bilinear b = geom::bilinear_border(grid[i], H, W);
      p[k] = geom::bilinear_sum(b, [=](int y, int x) { return ps[y * W + x]; });
      g[k] = geom::bilinear_sum(b, [=](int y, int x) { return gs[y * W + x]; });
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) {
        accumulate<false>(a, p[k], g[k], g[k] <= maxdepth, th);
        if (kStore) {
          if (pred_erp) pred_erp[base + i0 + k] = p[k];
          if (gt_erp) gt_erp[base + i0 + k] = g[k];
        }
      }
    }
  }
  block_fold(a, sh, slab + (long long)blockIdx.y * gridDim.x * kS, gridDim.x, blockIdx.x);
}

// One block per frame: metrics_final_kernel's fold on the frame's slab.
__global__ __launch_bounds__(NT) void erp_metrics_final_kernel(const double* __restrict__ slab, int nblocks, double* __restrict__ out) {
  __shared__ double sh[NT / 64][kS];
  __shared__ double fin[kS];
  fold_columns(slab + (long long)blockIdx.x * nblocks * kS, nblocks, sh, out + (long long)blockIdx.x * kS, fin);
}

// ---------------------------------------------------------------------------------------------------------------------
// F.interpolate(scale_factor=2, mode='bicubic', align_corners=True): the cubic convolution weights of torch (A = -0.75) at
// fraction t, for the taps at -1, 0, +1, +2.
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = (1.f - t) + 1.f, u = 1.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// source coordinate o * (in - 1) / (out - 1) of output index o: the integer part and the fraction.  The quotient of the exact
// integer product is formed in fp64, so that the last output lands exactly on the last input (fraction 0).
__device__ __forceinline__ int cubic_coord(int o, int in, int out, float& t) {
  const double r = (double)o * (double)(in - 1) / (double)(out - 1);
  const double f = floor(r);
  t = (float)(r - f);
  return (int)f;
}

__global__ __launch_bounds__(NT) void bicubic_up2_kernel(const float* __restrict__ src, float* __restrict__ dst, long long planes, int H,
                                                         int W) {
  const int Ho = 2 * H, Wo = 2 * W;
  const long long total = planes * Ho * Wo;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int ox = (int)(i % Wo);
    const long long r = i / Wo;
    const int oy = (int)(r % Ho);
    const float* __restrict__ s = src + (r / Ho) * H * W;
    float tx, ty, wx[4], wy[4];
    const int ix = cubic_coord(ox, W, Wo, tx), iy = cubic_coord(oy, H, Ho, ty);
    cubic_weights(tx, wx);
    cubic_weights(ty, wy);
    int xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = min(max(ix - 1 + k, 0), W - 1);  // border-clamped taps
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* __restrict__ row = s + (long long)min(max(iy - 1 + j, 0), H - 1) * W;
      const float h = row[xs[0]] * wx[0] + row[xs[1]] * wx[1] + row[xs[2]] * wx[2] + row[xs[3]] * wx[3];
      v += h * wy[j];
    }
    dst[i] = v;
  }
}

}  // namespace

extern "C" size_t mode_erp_depth_metrics_workspace_bytes(int frames, int H, int W) {
  if (frames < 0 || H <= 0 || W <= 0) return 0;
  return (size_t)frames * mode_masked_metrics_workspace_bytes((long long)H * W);
}

extern "C" int mode_erp_depth_metrics(const float* pred, const float* gt, const float* grid, int frames, int H, int W, float maxdepth,
                                      const mode_metrics_params* params, void* workspace, size_t workspace_bytes, double* out,
                                      float* pred_erp, float* gt_erp, mode_stream_t stream) {
  const char* who = "mode_erp_depth_metrics";
  MODE_REQUIRE(frames >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d", who, frames, H, W);
  MODE_REQUIRE(H == 2 * W, MODE_ERR_BAD_ARG, "%s: a Cassini frame is H = 2 W, got %d x %d", who, H, W);
  MODE_REQUIRE((long long)H * W < (1LL << 31) && frames <= 65535, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d (too large)", who, frames, H, W);
  MODE_REQUIRE(params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  Thresholds th;
  int rc = load_thresholds(params, th, who);
  if (rc != MODE_OK) return rc;
  if (frames == 0) return MODE_OK;
  MODE_REQUIRE(pred && gt && grid && out, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(grid) & 7) == 0, MODE_ERR_BAD_ARG, "%s: grid must be 8-byte aligned", who);
  MODE_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MODE_ERR_WORKSPACE,
               "%s: workspace missing or not 8-byte aligned", who);
  const size_t need = mode_erp_depth_metrics_workspace_bytes(frames, H, W);
  MODE_REQUIRE(workspace_bytes >= need, MODE_ERR_WORKSPACE, "%s: workspace of %zu B is too small (needs %zu B)", who, workspace_bytes, need);
  const int blocks = metric_blocks((long long)H * W);
  double* slab = static_cast<double*>(workspace);
  const float2* g2 = reinterpret_cast<const float2*>(grid);
  hipStream_t st = mode::as_stream(stream);
  if (pred_erp || gt_erp)
    hipLaunchKernelGGL(erp_metrics_partial_kernel<true>, dim3(blocks, frames), dim3(NT), 0, st, pred, gt, g2, H, W, maxdepth, th, slab,
                       pred_erp, gt_erp);
  else
    hipLaunchKernelGGL(erp_metrics_partial_kernel<false>, dim3(blocks, frames), dim3(NT), 0, st, pred, gt, g2, H, W, maxdepth, th, slab,
                       pred_erp, gt_erp);
  hipLaunchKernelGGL(erp_metrics_final_kernel, dim3(frames), dim3(NT), 0, st, slab, blocks, out);
  return mode::check_launch(who);
}

extern "C" int mode_bicubic_up2(const float* src, float* dst, int N, int C, int H, int W, mode_stream_t stream) {
  const char* who = "mode_bicubic_up2";
  MODE_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: non-positive size", who);
  MODE_REQUIRE(H < (1 << 20) && W < (1 << 20), MODE_ERR_BAD_ARG, "%s: bad size %d x %d (too large)", who, H, W);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(src && dst, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(src != dst, MODE_ERR_BAD_ARG, "%s: in-place operation is not possible", who);
  const long long planes = (long long)N * C, total = planes * 4 * H * W;
  const long long b = (total + NT - 1) / NT;
  const int blocks = (int)(b > 256 * 64 ? 256 * 64 : b);  // grid-stride beyond 64 blocks per CU
  hipLaunchKernelGGL(bicubic_up2_kernel, dim3(blocks), dim3(NT), 0, mode::as_stream(stream), src, dst, planes, H, W);
  return mode::check_launch(who);
}
