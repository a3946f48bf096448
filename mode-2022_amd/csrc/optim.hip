// Adam for all parameter tensors and parameter groups of a model in three launches (reference: train_disparity.py:293,
// optim.Adam(params, lr, betas=(0.9, 0.999)); include/mode_hip.h).
//
// prepare, launch 1: the sum of squares of the flat gradient in fp64 and the count of its non-finite elements, in the scheme of
//   metrics_internal.h: a grid that depends on n alone, every thread walks its quads in ascending order, a fixed butterfly and wave
//   order, one slab column per block.  prepare, launch 2 (one block): the columns folded in index order, then the DECISION -- skip or
//   step -- and what the update needs per group, formed in fp64 and rounded to fp32 as torch's single-tensor path forms it in Python.
// update, launch 3: one workgroup iteration per chunk of at most MODE_ADAM_CHUNK elements of one parameter tensor; fp32, unfused (no FMA
//   contraction: the element arithmetic is torch's, operation by operation), one square root and one division per element.
// No atomics, no ticket, no "last workgroup": the same inputs give the same bits on any stream.
#include "metrics_internal.h"

namespace {

using mode::metrics::metric_blocks;  // grid of the streaming pass, a function of n alone
using mode::metrics::NT;

constexpr int kMaxGrid = 2048;  // cap of the update's grid: 8 blocks per CU, grid-stride beyond
constexpr int kState = MODE_ADAM_STATE_DOUBLES, kGroup = MODE_ADAM_GROUP_DOUBLES;
constexpr int kDerived = 8;  // floats per group (and in the header in front of them) that prepare leaves for update

// What the update reads per group (floats 8 + 8 g .. of the derived part of the block).
struct Derived {
  float step_size, bc2_sqrt, clip, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
};
static_assert(sizeof(Derived) == kDerived * sizeof(float), "Derived is the block's per-group record");
static_assert(sizeof(mode_adam_segment) == 32 && sizeof(mode_adam_chunk) == 16, "table records as the header documents them");

__host__ __device__ inline float* derived_of(void* block, int n_groups) {
  return reinterpret_cast<float*>(static_cast<double*>(block) + kState + (long long)kGroup * n_groups);
}

__device__ __forceinline__ void square_into(double& s, unsigned& bad, float x) {
  s += (double)x * (double)x;
  bad += ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;  // inf or NaN
}

// Launch 1: block b leaves (sum of squares, non-finite count) in column b of the slab (slab[j * nblocks + b]).
__global__ __launch_bounds__(NT) void adam_sumsq_kernel(const float* __restrict__ grad, long long n, int vec, double* __restrict__ slab) {
  __shared__ double sh[NT / 64][2];
  double s = 0.0;
  unsigned bad = 0;
  const long long quads = (n + 3) / 4, full = n / 4;
  const long long stride = (long long)gridDim.x * NT;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < quads; q += stride) {
    const long long i0 = 4 * q;
    if (vec && q < full) {
      const float4 g = *reinterpret_cast<const float4*>(grad + i0);
      square_into(s, bad, g.x);
      square_into(s, bad, g.y);
      square_into(s, bad, g.z);
      square_into(s, bad, g.w);
    } else {  // the n % 4 tail, or a base that is not 16-byte aligned: the same quad element by element (same order, same bits)
      for (int k = 0; k < 4; ++k)
        if (i0 + k < n) square_into(s, bad, grad[i0 + k]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double c = (double)bad;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  if (lane == 0) {
    sh[wave][0] = s;
    sh[wave][1] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double v = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v += sh[w][threadIdx.x];
    slab[(long long)threadIdx.x * gridDim.x + blockIdx.x] = v;
  }
}

// Launch 2, one block: fold the columns in index order (thread t takes columns t, t + NT, ...; the fixed butterfly; the waves in
// index order), then decide and derive.
__global__ __launch_bounds__(NT) void adam_decide_kernel(const double* __restrict__ slab, int nblocks, double* __restrict__ block,
                                                         int n_groups, int guard) {
  __shared__ double sh[NT / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double step_old = block[MODE_ADAM_STEP], skipped_old = block[MODE_ADAM_SKIPPED];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += NT) v += slab[(long long)j * nblocks + b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();  // (also: every thread has read the old state before thread 0 writes the new one)
  double sumsq = sh[0][0], bad = sh[0][1];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) {
    sumsq += sh[w][0];
    bad += sh[w][1];
  }
  const double norm = sqrt(sumsq);
  const bool skip = guard != 0 && bad > 0.0;
  const double step = skip ? step_old : step_old + 1.0;
  float* derived = derived_of(block, n_groups);
  if (threadIdx.x == 0) {
    block[MODE_ADAM_STEP] = step;
    block[MODE_ADAM_SKIPPED] = skip ? skipped_old + 1.0 : skipped_old;
    block[MODE_ADAM_GRAD_NORM] = norm;
    block[MODE_ADAM_FOUND_INF] = bad > 0.0 ? 1.0 : 0.0;
    block[MODE_ADAM_NONFINITE] = bad;
    reinterpret_cast<int*>(derived)[0] = skip ? 1 : 0;
  }
  if (skip) return;
  for (int g = threadIdx.x; g < n_groups; g += NT) {
    const double* h = block + kState + (long long)kGroup * g;
    const double lr = h[0], beta1 = h[1], beta2 = h[2], eps = h[3], wd = h[4], max_norm = h[5];
    Derived d;
    d.step_size = (float)(lr / (1.0 - pow(beta1, step)));
    d.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, step));
    double clip = 1.0;
    if (max_norm > 0.0) {
      clip = max_norm / (norm + 1e-6);
      clip = clip > 1.0 ? 1.0 : clip;  // (a NaN norm stays a NaN coefficient, as torch.clamp leaves it)
    }
    d.clip = (float)clip;
    d.one_minus_beta1 = (float)(1.0 - beta1);
    d.beta2 = (float)beta2;
    d.one_minus_beta2 = (float)(1.0 - beta2);
    d.eps = (float)eps;
    d.weight_decay = (float)wd;
    reinterpret_cast<Derived*>(derived + kDerived)[g] = d;
  }
}

// One element, operation by operation as torch's single-tensor path (torch/optim/adam.py, _single_tensor_adam) performs it on fp32
// tensors: grad.add(param, alpha=weight_decay); exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2);
// denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, value=-step_size).  Every product and
// sum rounds on its own (no contraction into FMAs), the square root and the division are the correctly rounded ones.
template <bool kDecay, bool kLowWeight>
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const Derived& h) {
#pragma clang fp contract(off)
  g = g * h.clip;
  if (kDecay) g = g + h.weight_decay * p;
  const float diff = g - m;
  // aten's lerp: self + weight * diff for weight < 0.5, end - diff * (1 - weight) otherwise
  m = kLowWeight ? m + h.one_minus_beta1 * diff : g - diff * (1.f - h.one_minus_beta1);
  v = v * h.beta2;
  v = v + (h.one_minus_beta2 * g) * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p - h.step_size * (m / denom);
}

template <bool kDecay, bool kLowWeight>
__device__ __forceinline__ void adam_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           int count, const Derived& h) {
  // 16-byte accesses where the four addresses share their position inside a 16-byte line: `head` elements up to the first line
  // boundary and the tail behind the last whole line go one by one; with different positions the whole chunk does.
  const unsigned ph = (unsigned)((size_t)p >> 2) & 3u;
  const bool same = ph == ((unsigned)((size_t)g >> 2) & 3u) && ph == ((unsigned)((size_t)m >> 2) & 3u) && ph == ((unsigned)((size_t)v >> 2) & 3u);
  int head = same ? (int)((4u - ph) & 3u) : count;
  head = head < count ? head : count;
  const int nvec = (count - head) >> 2;
  // (vectorised over two iterations the compiler packs pairs of lanes' values and splits every 16-byte store into four)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int q = threadIdx.x; q < nvec; q += NT) {
    const int i = head + 4 * q;
    float4 pp = *reinterpret_cast<const float4*>(p + i);
    const float4 gg = *reinterpret_cast<const float4*>(g + i);
    float4 mm = *reinterpret_cast<const float4*>(m + i);
    float4 vv = *reinterpret_cast<const float4*>(v + i);
    adam_one<kDecay, kLowWeight>(pp.x, mm.x, vv.x, gg.x, h);
    adam_one<kDecay, kLowWeight>(pp.y, mm.y, vv.y, gg.y, h);
    adam_one<kDecay, kLowWeight>(pp.z, mm.z, vv.z, gg.z, h);
    adam_one<kDecay, kLowWeight>(pp.w, mm.w, vv.w, gg.w, h);
    *reinterpret_cast<float4*>(m + i) = mm;
    *reinterpret_cast<float4*>(v + i) = vv;
    *reinterpret_cast<float4*>(p + i) = pp;
  }
  // head [0, head) and tail [head + 4 nvec, count): fewer than 8 elements unless the whole chunk goes this way
  const int tail0 = head + 4 * nvec;
  const int nscalar = head + (count - tail0);
#pragma clang loop vectorize(disable) interleave(disable)
  for (int k = threadIdx.x; k < nscalar; k += NT) {
    const int i = k < head ? k : tail0 + (k - head);
    float pp = p[i], mm = m[i], vv = v[i];
    adam_one<kDecay, kLowWeight>(pp, mm, vv, g[i], h);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
}

// Launch 3: workgroup b takes the chunks b, b + gridDim.x, ...  Everything about a chunk is uniform over the workgroup.
__global__ __launch_bounds__(NT) void adam_update_kernel(const mode_adam_segment* __restrict__ segments, const mode_adam_chunk* __restrict__ chunks,
                                                         int n_chunks, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                         float* __restrict__ exp_avg_sq, const float* __restrict__ derived) {
  if (reinterpret_cast<const int*>(derived)[0] != 0) return;  // the step is skipped: nothing is written
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const mode_adam_chunk ch = chunks[c];
    const mode_adam_segment sg = segments[ch.seg];
    const Derived h = reinterpret_cast<const Derived*>(derived + kDerived)[sg.group];
    float* p = sg.param + (ch.off - sg.first);
    const float* g = grad + ch.off;
    float* m = exp_avg + ch.off;
    float* v = exp_avg_sq + ch.off;
    const bool low = h.one_minus_beta1 < 0.5f;
    if (h.weight_decay != 0.f) {
      if (low)
        adam_chunk<true, true>(p, g, m, v, ch.count, h);
      else
        adam_chunk<true, false>(p, g, m, v, ch.count, h);
    } else {
      if (low)
        adam_chunk<false, true>(p, g, m, v, ch.count, h);
      else
        adam_chunk<false, false>(p, g, m, v, ch.count, h);
    }
  }
}

}  // namespace

extern "C" size_t mode_adam_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  return (size_t)metric_blocks(n) * 2 * sizeof(double);
}

extern "C" size_t mode_adam_block_bytes(int n_groups) {
  if (n_groups <= 0) return 0;
  return (size_t)(kState + kGroup * (long long)n_groups) * sizeof(double) + (size_t)(kDerived + kDerived * (long long)n_groups) * sizeof(float);
}

extern "C" int mode_adam_prepare(const float* grad, long long n, void* workspace, size_t workspace_bytes, void* block, int n_groups,
                                 int skip_nonfinite, mode_stream_t stream) {
  const char* who = "mode_adam_prepare";
  MODE_REQUIRE(grad && block, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(n > 0 && n_groups > 0, MODE_ERR_BAD_ARG, "%s: bad sizes (n %lld, n_groups %d)", who, n, n_groups);
  MODE_REQUIRE(((size_t)block & 7) == 0 && ((size_t)grad & 3) == 0, MODE_ERR_BAD_ARG, "%s: misaligned block (8 bytes) or gradient (4 bytes)", who);
  MODE_REQUIRE(workspace && ((size_t)workspace & 7) == 0, MODE_ERR_WORKSPACE, "%s: workspace missing or not 8-byte aligned", who);
  MODE_REQUIRE(workspace_bytes >= mode_adam_workspace_bytes(n), MODE_ERR_WORKSPACE, "%s: workspace of %zu B is too small (needs %zu B)", who,
               workspace_bytes, mode_adam_workspace_bytes(n));
  const int blocks = metric_blocks(n);
  const int vec = ((size_t)grad & 15) == 0;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  hipLaunchKernelGGL(adam_sumsq_kernel, dim3(blocks), dim3(NT), 0, st, grad, n, vec, slab);
  hipLaunchKernelGGL(adam_decide_kernel, dim3(1), dim3(NT), 0, st, slab, blocks, static_cast<double*>(block), n_groups, skip_nonfinite);
  return mode::check_launch(who);
}

extern "C" int mode_adam_update(const mode_adam_segment* segments, int n_seg, const mode_adam_chunk* chunks, int n_chunks, const float* grad,
                                float* exp_avg, float* exp_avg_sq, void* block, int n_groups, mode_stream_t stream) {
  const char* who = "mode_adam_update";
  MODE_REQUIRE(segments && chunks, MODE_ERR_BAD_ARG, "%s: null pointer (segment or chunk table missing)", who);
  MODE_REQUIRE(grad && exp_avg && exp_avg_sq && block, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(n_seg > 0 && n_chunks > 0 && n_groups > 0, MODE_ERR_BAD_ARG, "%s: bad sizes (n_seg %d, n_chunks %d, n_groups %d)", who, n_seg,
               n_chunks, n_groups);
  MODE_REQUIRE(((size_t)block & 7) == 0 && (((size_t)grad | (size_t)exp_avg | (size_t)exp_avg_sq) & 3) == 0 &&
                   (((size_t)segments | (size_t)chunks) & 7) == 0,
               MODE_ERR_BAD_ARG, "%s: misaligned block, table (8 bytes) or flat buffer (4 bytes)", who);
  const int grid = n_chunks < kMaxGrid ? n_chunks : kMaxGrid;
  hipLaunchKernelGGL(adam_update_kernel, dim3(grid), dim3(NT), 0, mode::as_stream(stream), segments, chunks, n_chunks, grad, exp_avg, exp_avg_sq,
                     derived_of(block, n_groups));
  return mode::check_launch(who);
}
