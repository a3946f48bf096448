// Colour augmentation on the 8-bit ingest: the reference's inception_color_preproccess (dataloader/preprocess.py:33-46,
// 78-95) -- ToTensor, ColorJitter(0.4, 0.4, 0.4), Lighting(0.1, eigval, eigvec), Normalize -- on (N, H, W, 3) bytes, fused with the
// planar split of mode_frames_u8_ingest.  See include/mode_hip.h for the contract; in short, per image and in fp32, every operation
// rounded once and nothing contracted:
//   x = v / 255;  grey(x) = (0.2989 r + 0.587 g) + 0.114 b;  blend(a, b, k) = clamp(rho_k a + sigma_k b, 0, 1)
//   up to three operations in the image's own order: brightness blend(x, 0), contrast blend(x, mean of grey(x) over the image as x
//   stands when the step is reached), saturation blend(x, grey(x));  then x[c] += shift[c];  then (x[c] - mean[c]) / std[c].
// Two launches: augment_grey_kernel applies what precedes the contrast step and leaves per-block fp64 sums of grey (the scheme of
// metrics_internal.h: a thread walks its quads in ascending order, a fixed butterfly over the lanes, the waves in index order, one
// partial per block); augment_apply_kernel folds its image's partials in index order -- every block forms the same bits -- and runs
// the whole chain.  No atomics; the number of partials depends on H W alone.
// The draws (order, factors, shifts) are the host's: the kernels only read them.  An operation code selects a branch and nothing else,
// and a slot outside [0, slots) means "do not write this copy", so no value of the device-resident tables can move an access.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int kMaxPartials = 128;  // per image: one block per 256 quads up to 128 blocks (a 512 x 256 image), grid-stride beyond: a
                                   // 1024 x 512 panorama gives every thread four quads, over which a block's fixed work is spread
constexpr int kCoef = 9;           // rho, sigma of brightness, contrast, saturation; the three shifts
constexpr int kMaxDst = 2;         // slots of out one image can be written to
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2;

struct Image {
  int op[3];
  float rho[3], sigma[3], shift[3];
};

// (all of it depends on the image index alone: wave-uniform, scalar loads)
__device__ __forceinline__ Image load_image(const int* __restrict__ ops, const float* __restrict__ coef, long long n) {
  Image p;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p.op[i] = ops[3 * n + i];
    p.rho[i] = coef[kCoef * n + 2 * i];
    p.sigma[i] = coef[kCoef * n + 2 * i + 1];
    p.shift[i] = coef[kCoef * n + 6 + i];
  }
  return p;
}

// position of the (first) contrast step, 3 = none
__device__ __forceinline__ int contrast_at(const Image& p) {
  return p.op[0] == OP_CONTRAST ? 0 : (p.op[1] == OP_CONTRAST ? 1 : (p.op[2] == OP_CONTRAST ? 2 : 3));
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__device__ __forceinline__ float grey_of(float r, float g, float b) {
#pragma clang fp contract(off)
  const float rg = 0.2989f * r + 0.587f * g;
  return rg + 0.114f * b;
}

__device__ __forceinline__ float blend(float a, float b, float rho, float sigma) {
#pragma clang fp contract(off)
  const float u = rho * a, v = sigma * b;
  return clamp01(u + v);
}

// steps [from, to) of the image's order on one pixel; m: the contrast mean (read by a contrast step only).  The three positions are
// unrolled with a predicate each, so that the image's tables stay in (scalar) registers: indexed by a run-time position they
// would be moved to memory.
__device__ __forceinline__ void run_steps(const Image& p, int from, int to, float m, float& r, float& g, float& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i < from || i >= to) continue;
    const int op = p.op[i];
    if (op == OP_BRIGHTNESS) {
      r = blend(r, 0.f, p.rho[0], p.sigma[0]);
      g = blend(g, 0.f, p.rho[0], p.sigma[0]);
      b = blend(b, 0.f, p.rho[0], p.sigma[0]);
    } else if (op == OP_CONTRAST) {
      r = blend(r, m, p.rho[1], p.sigma[1]);
      g = blend(g, m, p.rho[1], p.sigma[1]);
      b = blend(b, m, p.rho[1], p.sigma[1]);
    } else if (op == OP_SATURATION) {
      const float y = grey_of(r, g, b);
      r = blend(r, y, p.rho[2], p.sigma[2]);
      g = blend(g, y, p.rho[2], p.sigma[2]);
      b = blend(b, y, p.rho[2], p.sigma[2]);
    }
  }
}

// ToTensor of the 256 byte values, once per block: s_unit[v] = v / 255 (IEEE division)
__device__ __forceinline__ void load_unit(float* s_unit) {
#pragma clang fp contract(off)
  s_unit[threadIdx.x] = (float)threadIdx.x / 255.0f;  // NT == 256
}

// four pixels = three dwords of interleaved bytes
struct Raw {
  unsigned w0, w1, w2;
};

__device__ __forceinline__ Raw load_raw(const unsigned* __restrict__ src) { return Raw{src[0], src[1], src[2]}; }

// -> ToTensor values per channel
__device__ __forceinline__ void unpack_quad(const Raw& w, const float* s_unit, float* r, float* g, float* b) {
  const unsigned w0 = w.w0, w1 = w.w1, w2 = w.w2;
  r[0] = s_unit[w0 & 255u], r[1] = s_unit[w0 >> 24], r[2] = s_unit[(w1 >> 16) & 255u], r[3] = s_unit[(w2 >> 8) & 255u];
  g[0] = s_unit[(w0 >> 8) & 255u], g[1] = s_unit[w1 & 255u], g[2] = s_unit[w1 >> 24], g[3] = s_unit[(w2 >> 16) & 255u];
  b[0] = s_unit[(w0 >> 16) & 255u], b[1] = s_unit[(w1 >> 8) & 255u], b[2] = s_unit[w2 & 255u], b[3] = s_unit[w2 >> 24];
}

// the block's sum in a fixed order: butterfly over the lanes, then the waves in index order; valid in every thread after the call
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();  // (sh may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) s += sh[w];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Launch 1.  grid = (P, min(N, 65535)); block x of image n sums grey over its quads x NT + t, (x + P) NT + t, ... into partials[n P + x].
__global__ __launch_bounds__(NT) void augment_grey_kernel(const unsigned* __restrict__ images, const int* __restrict__ ops,
                                                          const float* __restrict__ coef, int N, int quads, double* __restrict__ partials) {
  __shared__ float s_unit[NT];
  __shared__ double s_sum[NT / 64];
  load_unit(s_unit);
  __syncthreads();
  const int P = gridDim.x;
  for (long long n = blockIdx.y; n < N; n += gridDim.y) {
    const Image p = load_image(ops, coef, n);
    const int pc = contrast_at(p);
    if (pc == 3) continue;  // no contrast step: nobody reads this image's partials
    const unsigned* img = images + 3 * n * quads;
    double acc = 0.0;
    int q = blockIdx.x * NT + threadIdx.x;
    Raw w = q < quads ? load_raw(img + 3LL * q) : Raw{0u, 0u, 0u};
    while (q < quads) {
      const int qn = q + P * NT;  // the next quad's bytes are on their way while this one is worked on
      const Raw wn = qn < quads ? load_raw(img + 3LL * qn) : Raw{0u, 0u, 0u};
      float r[4], g[4], b[4];
      unpack_quad(w, s_unit, r, g, b);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        run_steps(p, 0, pc, 0.f, r[e], g[e], b[e]);
        acc += (double)grey_of(r[e], g[e], b[e]);
      }
      w = wn;
      q = qn;
    }
    const double s = block_sum(acc, s_sum);
    if (threadIdx.x == 0) partials[n * P + blockIdx.x] = s;
  }
}

// Launch 2.  Same grid.  Every block folds the P partials of its image in index order (thread t: columns t, t + NT), divides by H W,
// rounds once to fp32, and runs the whole chain on its quads: one 16-byte store per colour plane.
__global__ __launch_bounds__(NT) void augment_apply_kernel(const unsigned* __restrict__ images, const int* __restrict__ ops,
                                                           const float* __restrict__ coef, const int* __restrict__ dst, int ndst, int N,
                                                           int quads, int slots, const double* __restrict__ partials, float* __restrict__ out,
                                                           float* __restrict__ means) {
#pragma clang fp contract(off)
  __shared__ float s_unit[NT];
  __shared__ double s_sum[NT / 64];
  load_unit(s_unit);
  __syncthreads();
  const int P = gridDim.x;
  const long long hw = 4LL * quads;
  for (long long n = blockIdx.y; n < N; n += gridDim.y) {
    const Image p = load_image(ops, coef, n);
    // up to kMaxDst slots per image; -1: not a slot of out, nothing is written there
    long long slot[kMaxDst];
#pragma unroll
    for (int j = 0; j < kMaxDst; ++j) {
      const long long s = j < ndst ? (dst ? (long long)dst[n * ndst + j] : n) : -1;
      slot[j] = (s >= 0 && s < slots) ? s : -1;
    }
    const bool written = slot[0] >= 0 || slot[1] >= 0;
    const unsigned* img = images + 3 * n * quads;
    int q = blockIdx.x * NT + threadIdx.x;
    Raw w = written && q < quads ? load_raw(img + 3LL * q) : Raw{0u, 0u, 0u};  // (in flight during the fold)
    float m = 0.f;
    if (contrast_at(p) != 3) {
      double v = 0.0;
      for (int c = threadIdx.x; c < P; c += NT) v += partials[n * P + c];
      m = (float)(block_sum(v, s_sum) / (double)hw);
    }
    if (means && blockIdx.x == 0 && threadIdx.x == 0) means[n] = m;
    if (!written) continue;
    while (q < quads) {
      const int qn = q + P * NT;
      const Raw wn = qn < quads ? load_raw(img + 3LL * qn) : Raw{0u, 0u, 0u};
      float r[4], g[4], b[4];
      unpack_quad(w, s_unit, r, g, b);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        run_steps(p, 0, 3, m, r[e], g[e], b[e]);
        r[e] = ((r[e] + p.shift[0]) - 0.485f) / 0.229f;  // Lighting (no clamp), then Normalize with the fp32 ImageNet statistics
        g[e] = ((g[e] + p.shift[1]) - 0.456f) / 0.224f;
        b[e] = ((b[e] + p.shift[2]) - 0.406f) / 0.225f;
      }
#pragma unroll
      for (int j = 0; j < kMaxDst; ++j) {
        if (slot[j] < 0) continue;
        float* d = out + slot[j] * 3 * hw + 4LL * q;
        *reinterpret_cast<float4*>(d) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(d + hw) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(d + 2 * hw) = make_float4(b[0], b[1], b[2], b[3]);
      }
      w = wn;
      q = qn;
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// n * 3 * H * W < 2^31 without forming a product that could overflow (n >= 0, H, W > 0)
bool fits31(long long n, int H, int W) {
  const long long lim = ((1LL << 31) - 1) / 3, hw = (long long)H * W;
  return hw <= lim && n <= lim / hw;
}

// partials per image: a function of H W alone
int partials_of(int H, int W) {
  const long long quads = ((long long)H * W + 3) / 4, b = (quads + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b));
}

}  // namespace

extern "C" size_t mode_images_u8_augment_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * (size_t)partials_of(H, W) * sizeof(double);
}

extern "C" int mode_images_u8_augment(const uint8_t* images_u8, const int32_t* ops, const float* coef, const int32_t* dst, int ndst, int N,
                                      int H, int W, int slots, float* out, float* means, void* workspace, size_t workspace_bytes,
                                      mode_stream_t stream) {
  const char* who = "mode_images_u8_augment";
  MODE_REQUIRE(N >= 0 && slots >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d (%d slots) x %d x %d", who, N, slots, H, W);
  MODE_REQUIRE(fits31(N, H, W) && fits31(slots, H, W), MODE_ERR_BAD_ARG,
               "%s: bad size %d (%d slots) x %d x %d (too large: 3 N H W or 3 slots H W >= 2^31)", who, N, slots, H, W);
  MODE_REQUIRE(ndst >= 1 && ndst <= kMaxDst, MODE_ERR_BAD_ARG, "%s: %d slots per image (1 or %d)", who, ndst, kMaxDst);
  MODE_REQUIRE(((long long)H * W) % 4 == 0, MODE_ERR_BAD_ARG, "%s: H W = %d x %d is not a multiple of 4", who, H, W);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(images_u8 && ops && coef && out && workspace, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(aligned(images_u8, 4) && aligned(ops, 4) && aligned(coef, 4) && aligned(dst, 4) && aligned(means, 4), MODE_ERR_BAD_ARG,
               "%s: images, tables and means must be 4-byte aligned", who);
  MODE_REQUIRE(aligned(out, 16), MODE_ERR_BAD_ARG, "%s: out must be 16-byte aligned", who);
  MODE_REQUIRE(aligned(workspace, 8), MODE_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned", who);
  const size_t need = mode_images_u8_augment_workspace_bytes(N, H, W);
  MODE_REQUIRE(workspace_bytes >= need, MODE_ERR_BAD_ARG, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const int quads = (int)((long long)H * W / 4);
  const dim3 grid((unsigned)partials_of(H, W), (unsigned)std::min(N, 65535));
  hipStream_t st = mode::as_stream(stream);
  const unsigned* images = reinterpret_cast<const unsigned*>(images_u8);
  double* partials = static_cast<double*>(workspace);
  hipLaunchKernelGGL(augment_grey_kernel, grid, dim3(NT), 0, st, images, ops, coef, N, quads, partials);
  const int rc = mode::check_launch(who);
  if (rc != MODE_OK) return rc;
  hipLaunchKernelGGL(augment_apply_kernel, grid, dim3(NT), 0, st, images, ops, coef, dst, dst ? ndst : 1, N, quads, slots,
                     partials, out, means);
  return mode::check_launch(who);
}
