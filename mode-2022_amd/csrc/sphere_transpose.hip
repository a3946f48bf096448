// Plane transpose: the windowed spherical kernels run with every access coalesced when the planes are stored with the
// shift-invariant (longitude) axis contiguous, which for the Cassini layout is the transpose.
#include <algorithm>

#include "common.h"

namespace {

// out[p][w][h] = in[p][h][w] for P planes of H x W: 32x32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void transpose_planes_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W) {
  __shared__ float tile[32][33];
  const long long plane = (long long)blockIdx.z * H * W;
  const int w0 = blockIdx.x * 32, h0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int h = h0 + ty + i, w = w0 + tx;
    if (h < H && w < W) tile[ty + i][tx] = in[plane + (long long)h * W + w];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int w = w0 + ty + i, h = h0 + tx;
    if (h < H && w < W) out[plane + (long long)w * H + h] = tile[tx][ty + i];
  }
}

}  // namespace

// out (P, W, H) = in (P, H, W) transposed plane by plane (P = B*C).  The windowed kernels run with every access coalesced when
// the planes are stored with the shift-invariant (longitude) axis contiguous, which for the Cassini layout is the transpose.
extern "C" int mode_transpose_planes(const float* in, float* out, long long planes, int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(planes >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "mode_transpose_planes: bad size");
  if (planes == 0) return MODE_OK;
  MODE_REQUIRE(in && out, MODE_ERR_BAD_ARG, "mode_transpose_planes: null pointer");
  hipStream_t st = mode::as_stream(stream);
  for (long long p0 = 0; p0 < planes; p0 += 65535) {
    const int np = (int)std::min<long long>(65535, planes - p0);
    hipLaunchKernelGGL(transpose_planes_kernel, dim3(mode::cdiv(W, 32), mode::cdiv(H, 32), np), dim3(256), 0, st,
                       in + p0 * (long long)H * W, out + p0 * (long long)H * W, H, W);
  }
  return mode::check_launch("mode_transpose_planes");
}
