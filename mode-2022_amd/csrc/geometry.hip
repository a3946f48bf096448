// Export-stage geometry of the disparity network: disparity -> depth, Cassini re-projections and
// the depth view transform with its z-buffer, gfx950.
//
// Reference (host numpy + a CPU<->GPU ping-pong per call + a sequential numba loop):
//   save_output_disparity_stage.py:105-160   disp2depth
//   utils/geometry.py:7-45, 48-96, 160-198   cassini2Equirec / rotateCassini / erp2rect_cassini: angle maps on the host,
//                                            then F.grid_sample(bilinear, align_corners=True, padding_mode='border')
//   utils/geometry.py:99-145                 depthViewTransWithConf: 3D re-projection of every pixel
//   utils/geometry.py:148-156                __iterPixels_with_conf: sequential z-buffer scatter (numba)
// Here the maps the reference builds with numpy stay on the host (they depend on the image size only and are cached by the
// caller); everything per pixel runs on the GPU with no host round trip.  All three kernels are HBM-bound elementwise /
// gather / scatter work: 4-16 bytes per pixel and direction.
#include "common.h"
#include "geometry_internal.h"

namespace {

namespace geom = mode::geom;
constexpr int NT = 256;

// The per-pixel arithmetic lives in geometry_internal.h (shared with the multi-view hand-off, multiview.hip).
using geom::Bilinear;
using geom::ViewXform;

// disparity -> depth by the sine rule (geom::sine_rule_depth)
__global__ __launch_bounds__(NT) void disp2depth_kernel(const float* __restrict__ disp, float* __restrict__ depth, long long n, int W,
                                                        float baseline) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int j = (int)(i % W);
    depth[i] = geom::sine_rule_depth(disp[i], j, W, baseline);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// F.grid_sample(src, grid, mode='bilinear', padding_mode='border', align_corners=True) for (N, C, Hs, Ws) -> (N, C, Ho, Wo);
// grid (Ng, Ho, Wo, 2) with Ng = N or 1 (shared by all samples: the reference repeat_interleaves one grid).
__global__ __launch_bounds__(NT) void grid_sample_border_kernel(const float* __restrict__ src, const float* __restrict__ grid,
                                                                float* __restrict__ dst, int N, int C, int Hs, int Ws, int Ho,
                                                                int Wo, int Ng) {
  const long long npix = (long long)Ho * Wo;
  const long long total = (long long)N * npix;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int n = (int)(i / npix);
    const long long p = i - (long long)n * npix;
    const float2 g = reinterpret_cast<const float2*>(grid)[(Ng == 1 ? 0 : (long long)n * npix) + p];
    const Bilinear b = geom::bilinear_border(g, Hs, Ws);
    const float* sp = src + (long long)n * C * Hs * Ws;
    float* dp = dst + (long long)n * C * npix + p;
    for (int c = 0; c < C; ++c) {
      const float* s = sp + (long long)c * Hs * Ws;
      dp[(long long)c * npix] = geom::bilinear_sum(b, [=](int y, int x) { return s[(long long)y * Ws + x]; });
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// depthViewTransWithConf: pass 1 projects every source pixel (geom::project_pixel) and keeps the reference's survivor of every
// target by a 64-bit atomic min of geom::zkey; pass 2 (geom::resolve_key) turns the keys into depth and confidence.
__global__ __launch_bounds__(NT) void view_trans_scatter_kernel(const float* __restrict__ view1, const float* __restrict__ trig,
                                                                unsigned long long* __restrict__ keys, int H, int W, ViewXform xf) {
  const long long n = (long long)H * W;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < n; idx += (long long)gridDim.x * NT) {
    double r2;
    long long tgt;
    const int i = (int)(idx / W), j = (int)(idx - (long long)i * W);
    if (geom::project_pixel(view1[idx], trig[j], trig[W + j], trig[2 * W + i], trig[2 * W + H + i], xf, H, W, r2, tgt))
      atomicMin(keys + tgt, geom::zkey(r2, idx, n));
  }
}

// the two halves on their own (tests, and callers that bring their own projection): projection to (r2, target index or -1) ...
__global__ __launch_bounds__(NT) void view_project_kernel(const float* __restrict__ view1, const float* __restrict__ trig,
                                                          double* __restrict__ r2_out, int* __restrict__ tgt_out, int H, int W, ViewXform xf) {
  const long long n = (long long)H * W;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < n; idx += (long long)gridDim.x * NT) {
    double r2 = 0.0;
    long long tgt = -1;
    const int i = (int)(idx / W), j = (int)(idx - (long long)i * W);
    const bool ok = geom::project_pixel(view1[idx], trig[j], trig[W + j], trig[2 * W + i], trig[2 * W + H + i], xf, H, W, r2, tgt);
    r2_out[idx] = r2;
    tgt_out[idx] = ok ? (int)tgt : -1;
  }
}

// ... and the scatter of given (r2, target) pairs
__global__ __launch_bounds__(NT) void zbuffer_scatter_kernel(const double* __restrict__ r2, const int* __restrict__ tgt,
                                                             unsigned long long* __restrict__ keys, long long n) {
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < n; idx += (long long)gridDim.x * NT) {
    const int t = tgt[idx];
    if (t >= 0 && t < n && r2[idx] < 100000.0) atomicMin(keys + t, geom::zkey(r2[idx], idx, n));
  }
}

__global__ __launch_bounds__(NT) void view_trans_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                const float* __restrict__ conf1, float* __restrict__ view2,
                                                                float* __restrict__ conf2, long long n) {
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < n; idx += (long long)gridDim.x * NT) {
    const float2 vc = geom::resolve_key(keys[idx], conf1, n);
    view2[idx] = vc.x;
    conf2[idx] = vc.y;
  }
}

int grid_for(long long n) { return (int)std::min<long long>(mode::cdiv(n, NT), 8LL * kNumCU); }

}  // namespace

extern "C" int mode_disp2depth(const float* disp, float* depth, int H, int W, float baseline, mode_stream_t stream) {
  MODE_REQUIRE(H >= 0 && W > 0, MODE_ERR_BAD_ARG, "mode_disp2depth: bad size %dx%d", H, W);
  if (H == 0) return MODE_OK;
  MODE_REQUIRE(disp && depth, MODE_ERR_BAD_ARG, "mode_disp2depth: null pointer");
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(disp2depth_kernel, dim3(grid_for(n)), dim3(NT), 0, mode::as_stream(stream), disp, depth, n, W, baseline);
  return mode::check_launch("mode_disp2depth");
}

extern "C" int mode_grid_sample_border(const float* src, const float* grid, float* dst, int N, int C, int Hs, int Ws, int Ho, int Wo,
                                       int grids, mode_stream_t stream) {
  MODE_REQUIRE(N >= 0 && C > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, MODE_ERR_BAD_ARG, "mode_grid_sample_border: non-positive size");
  MODE_REQUIRE(grids == 1 || grids == N, MODE_ERR_BAD_ARG, "mode_grid_sample_border: %d grids for %d samples", grids, N);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(src && grid && dst, MODE_ERR_BAD_ARG, "mode_grid_sample_border: null pointer");
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(grid) & 7) == 0, MODE_ERR_UNSUPPORTED, "mode_grid_sample_border: grid must be 8-byte aligned");
  const long long n = (long long)N * Ho * Wo;
  hipLaunchKernelGGL(grid_sample_border_kernel, dim3(grid_for(n)), dim3(NT), 0, mode::as_stream(stream), src, grid, dst, N, C, Hs, Ws,
                     Ho, Wo, grids);
  return mode::check_launch("mode_grid_sample_border");
}

extern "C" size_t mode_depth_view_trans_workspace_bytes(int H, int W) {
  return H > 0 && W > 0 ? (size_t)H * W * sizeof(unsigned long long) : 0;
}

extern "C" int mode_depth_view_trans(const float* view1, const float* conf1, const float* trig, const double* R, const double* t,
                                     float* view2, float* conf2, void* workspace, int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), MODE_ERR_BAD_ARG, "mode_depth_view_trans: bad size %dx%d", H, W);
  MODE_REQUIRE(view1 && conf1 && trig && R && t && view2 && conf2, MODE_ERR_BAD_ARG, "mode_depth_view_trans: null pointer");
  MODE_REQUIRE(workspace, MODE_ERR_WORKSPACE, "mode_depth_view_trans: workspace required");
  MODE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MODE_ERR_UNSUPPORTED, "mode_depth_view_trans: unaligned workspace");
  hipStream_t st = mode::as_stream(stream);
  const long long n = (long long)H * W;
  ViewXform xf;
  for (int i = 0; i < 9; ++i) xf.R[i] = R[i];
  for (int i = 0; i < 3; ++i) xf.t[i] = t[i];
  int frc = mode::fill_words(workspace, 0xffffffffu, 2 * (size_t)n, st, "mode_depth_view_trans");  // all keys = +inf (a kernel, not hipMemsetAsync: common.h)
  if (frc != MODE_OK) return frc;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(view_trans_scatter_kernel, dim3(grid_for(n)), dim3(NT), 0, st, view1, trig, keys, H, W, xf);
  hipLaunchKernelGGL(view_trans_resolve_kernel, dim3(grid_for(n)), dim3(NT), 0, st, keys, conf1, view2, conf2, n);
  return mode::check_launch("mode_depth_view_trans");
}

// The two halves of mode_depth_view_trans on their own: per-source projection (r2 as float64, target index i*W + j, or -1 for a
// source that takes no part), and the z-buffer over given (r2, target) pairs with the reference's exact overwrite rule.
extern "C" int mode_depth_view_project(const float* view1, const float* trig, const double* R, const double* t, double* r2, int32_t* target,
                                       int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), MODE_ERR_BAD_ARG, "mode_depth_view_project: bad size %dx%d", H, W);
  MODE_REQUIRE(view1 && trig && R && t && r2 && target, MODE_ERR_BAD_ARG, "mode_depth_view_project: null pointer");
  ViewXform xf;
  for (int i = 0; i < 9; ++i) xf.R[i] = R[i];
  for (int i = 0; i < 3; ++i) xf.t[i] = t[i];
  hipLaunchKernelGGL(view_project_kernel, dim3(grid_for((long long)H * W)), dim3(NT), 0, mode::as_stream(stream), view1, trig, r2, target, H,
                     W, xf);
  return mode::check_launch("mode_depth_view_project");
}

extern "C" int mode_zbuffer(const double* r2, const int32_t* target, const float* conf1, float* view2, float* conf2, void* workspace,
                            long long n, mode_stream_t stream) {
  MODE_REQUIRE(n > 0 && n < (1LL << 31), MODE_ERR_BAD_ARG, "mode_zbuffer: bad size");
  MODE_REQUIRE(r2 && target && conf1 && view2 && conf2, MODE_ERR_BAD_ARG, "mode_zbuffer: null pointer");
  MODE_REQUIRE(workspace, MODE_ERR_WORKSPACE, "mode_zbuffer: workspace required");
  hipStream_t st = mode::as_stream(stream);
  int frc = mode::fill_words(workspace, 0xffffffffu, 2 * (size_t)n, st, "mode_zbuffer");  // all keys = +inf (a kernel, not hipMemsetAsync: common.h)
  if (frc != MODE_OK) return frc;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(zbuffer_scatter_kernel, dim3(grid_for(n)), dim3(NT), 0, st, r2, target, keys, n);
  hipLaunchKernelGGL(view_trans_resolve_kernel, dim3(grid_for(n)), dim3(NT), 0, st, keys, conf1, view2, conf2, n);
  return mode::check_launch("mode_zbuffer");
}
