// Masked evaluation metrics and the SILog training loss (reference: utils/evaluation.py, train_fusion.py:82-87): see include/mode_hip.h.
//
// One streaming pass forms every statistic the reference's ten metric functions reduce, over the elements a uint8 mask selects:
// counts, fp64 sums of the per-element fp32 terms as torch forms them, the NaN-propagating maximum of |pred - gt| and the threshold
// counts.  Deterministic by construction: element quad q (elements 4q .. 4q + 3) belongs to thread q % T of a grid of T threads that
// depends on n alone, every thread walks its quads in ascending order, a block reduces its threads by a fixed butterfly and a fixed
// wave order, writes its partials to its own slab column, and a second single-block launch folds the columns in index order.  No
// atomics; the same n gives the same bits on any stream, whatever the placement or arrival order of the blocks.
#include "metrics_internal.h"

namespace {

using namespace mode::metrics;  // the shared scheme: Acc, accumulate, block_fold, fold_columns, metric_blocks (metrics_internal.h)

// Stage 1: block b leaves its statistics in column b of the slab (slab[j * nblocks + b]).
template <bool kMask, bool kLogOnly>
__global__ __launch_bounds__(NT) void metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const unsigned char* __restrict__ mask, long long n, int vec,
                                                             Thresholds th, double* __restrict__ slab) {
  __shared__ double sh[NT / 64][kS];
  Acc a = {};
  const long long quads = (n + 3) / 4, full = n / 4;
  const long long stride = (long long)gridDim.x * NT;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < quads; q += stride) {
    const long long i0 = 4 * q;
    if (vec && q < full) {  // 16-B loads of pred / gt, 4 mask bytes (every base aligned: decided on the host)
      const float4 p = *reinterpret_cast<const float4*>(pred + i0);
      const float4 g = *reinterpret_cast<const float4*>(gt + i0);
      unsigned m = 0x01010101u;
      if (kMask) m = *reinterpret_cast<const unsigned*>(mask + i0);
      accumulate<kLogOnly>(a, p.x, g.x, (m & 0xffu) != 0, th);
      accumulate<kLogOnly>(a, p.y, g.y, (m & 0xff00u) != 0, th);
      accumulate<kLogOnly>(a, p.z, g.z, (m & 0xff0000u) != 0, th);
      accumulate<kLogOnly>(a, p.w, g.w, (m & 0xff000000u) != 0, th);
    } else {  // the same quad element by element: the n % 4 tail, or bases that are not aligned (same order, same bits)
      for (int k = 0; k < 4; ++k) {
        const long long i = i0 + k;
        if (i < n) accumulate<kLogOnly>(a, pred[i], gt[i], kMask ? mask[i] != 0 : true, th);
      }
    }
  }
  block_fold(a, sh, slab, gridDim.x, blockIdx.x);
}

// Stage 2, one block: fold the columns (fold_columns), write the statistic vector and, for the loss,
// loss = sum l^2 / n - lamda (sum l / n)^2 (NaN for n = 0, as torch's mean of nothing).
__global__ __launch_bounds__(NT) void metrics_final_kernel(const double* __restrict__ slab, int nblocks, double* __restrict__ out,
                                                           float* __restrict__ loss, float lamda) {
  __shared__ double sh[NT / 64][kS];
  __shared__ double fin[kS];
  fold_columns(slab, nblocks, sh, out, fin);
  if (loss) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const double nb = fin[MODE_METRICS_N_BOTH];
      const double m1 = fin[MODE_METRICS_SUM_LOG] / nb, m2 = fin[MODE_METRICS_SUM_LOG2] / nb;
      loss[0] = (float)(m2 - (double)lamda * m1 * m1);
    }
  }
}

// d loss / d pred = gloss * (2 / n) (l - lamda sum l / n) / p on the selected elements (mask, gt > 0, pred > 0), exactly 0 elsewhere.
__device__ __forceinline__ float silog_grad(float p, float g, bool sel, double c, double mean_l) {
  if (!sel || !(g > 0.f) || !(p > 0.f)) return 0.f;
  const double l = log((double)p) - log((double)g);
  return (float)(c * (l - mean_l) / (double)p);
}

template <bool kMask>
__global__ __launch_bounds__(NT) void silog_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const unsigned char* __restrict__ mask, long long n, int vec, float lamda,
                                                       const double* __restrict__ stats, const float* __restrict__ gloss,
                                                       float* __restrict__ gpred) {
  const double nb = stats[MODE_METRICS_N_BOTH];
  // nb == 0 selects nothing: c and mean_l are never used (the gradient is all zeros, as torch's of a mean over nothing)
  const double c = nb > 0.0 ? (double)gloss[0] * 2.0 / nb : 0.0;
  const double mean_l = nb > 0.0 ? (double)lamda * stats[MODE_METRICS_SUM_LOG] / nb : 0.0;
  const long long quads = (n + 3) / 4, full = n / 4;
  const long long stride = (long long)gridDim.x * NT;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < quads; q += stride) {
    const long long i0 = 4 * q;
    if (vec && q < full) {
      const float4 p = *reinterpret_cast<const float4*>(pred + i0);
      const float4 g = *reinterpret_cast<const float4*>(gt + i0);
      unsigned m = 0x01010101u;
      if (kMask) m = *reinterpret_cast<const unsigned*>(mask + i0);
      float4 o;
      o.x = silog_grad(p.x, g.x, (m & 0xffu) != 0, c, mean_l);
      o.y = silog_grad(p.y, g.y, (m & 0xff00u) != 0, c, mean_l);
      o.z = silog_grad(p.z, g.z, (m & 0xff0000u) != 0, c, mean_l);
      o.w = silog_grad(p.w, g.w, (m & 0xff000000u) != 0, c, mean_l);
      *reinterpret_cast<float4*>(gpred + i0) = o;
    } else {
      for (int k = 0; k < 4; ++k) {
        const long long i = i0 + k;
        if (i < n) gpred[i] = silog_grad(pred[i], gt[i], kMask ? mask[i] != 0 : true, c, mean_l);
      }
    }
  }
}

int vec_ok(const void* a, const void* b, const void* c, const void* mask) {
  const size_t al = (size_t)a | (size_t)b | (size_t)c;
  return (al & 15) == 0 && ((size_t)mask & 3) == 0;
}

int check_common(const char* who, const float* pred, const float* gt, long long n, const void* workspace, size_t workspace_bytes) {
  MODE_REQUIRE(n >= 0, MODE_ERR_BAD_ARG, "%s: negative size %lld", who, n);
  MODE_REQUIRE((pred && gt) || n == 0, MODE_ERR_BAD_ARG, "%s: null pointer", who);  // an empty tensor may have no storage
  MODE_REQUIRE(workspace && ((size_t)workspace & 7) == 0, MODE_ERR_WORKSPACE, "%s: workspace missing or not 8-byte aligned", who);
  MODE_REQUIRE(workspace_bytes >= mode_masked_metrics_workspace_bytes(n), MODE_ERR_WORKSPACE, "%s: workspace of %zu B is too small (needs %zu B)",
               who, workspace_bytes, mode_masked_metrics_workspace_bytes(n));
  return MODE_OK;
}

}  // namespace

extern "C" size_t mode_masked_metrics_workspace_bytes(long long n) {
  if (n < 0) return 0;
  return (size_t)metric_blocks(n) * kS * sizeof(double);
}

extern "C" int mode_masked_metrics(const float* pred, const float* gt, const uint8_t* mask, long long n, const mode_metrics_params* params,
                                   void* workspace, size_t workspace_bytes, double* out, mode_stream_t stream) {
  const char* who = "mode_masked_metrics";
  int rc = check_common(who, pred, gt, n, workspace, workspace_bytes);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(params && out, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  Thresholds th;
  rc = load_thresholds(params, th, who);
  if (rc != MODE_OK) return rc;
  const int blocks = metric_blocks(n);
  const int vec = vec_ok(pred, gt, nullptr, mask);
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  if (mask)
    hipLaunchKernelGGL((metrics_partial_kernel<true, false>), dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, th, slab);
  else
    hipLaunchKernelGGL((metrics_partial_kernel<false, false>), dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, th, slab);
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(NT), 0, st, slab, blocks, out, nullptr, 0.f);
  return mode::check_launch(who);
}

extern "C" int mode_silog_loss_fwd(const float* pred, const float* gt, const uint8_t* mask, long long n, float lamda, void* workspace,
                                   size_t workspace_bytes, double* stats, float* loss, mode_stream_t stream) {
  const char* who = "mode_silog_loss_fwd";
  int rc = check_common(who, pred, gt, n, workspace, workspace_bytes);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  Thresholds th = {};
  const int blocks = metric_blocks(n);
  const int vec = vec_ok(pred, gt, nullptr, mask);
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  if (mask)
    hipLaunchKernelGGL((metrics_partial_kernel<true, true>), dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, th, slab);
  else
    hipLaunchKernelGGL((metrics_partial_kernel<false, true>), dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, th, slab);
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(NT), 0, st, slab, blocks, stats, loss, lamda);
  return mode::check_launch(who);
}

extern "C" int mode_silog_loss_bwd(const float* pred, const float* gt, const uint8_t* mask, long long n, float lamda, const double* stats,
                                   const float* gloss, float* gpred, mode_stream_t stream) {
  const char* who = "mode_silog_loss_bwd";
  MODE_REQUIRE(n >= 0, MODE_ERR_BAD_ARG, "%s: negative size %lld", who, n);
  MODE_REQUIRE((pred && gt && gpred) || n == 0, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(stats && gloss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  if (n == 0) return MODE_OK;
  const int blocks = metric_blocks(n);
  const int vec = vec_ok(pred, gt, gpred, mask);
  hipStream_t st = mode::as_stream(stream);
  if (mask)
    hipLaunchKernelGGL(silog_bwd_kernel<true>, dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, lamda, stats, gloss, gpred);
  else
    hipLaunchKernelGGL(silog_bwd_kernel<false>, dim3(blocks), dim3(NT), 0, st, pred, gt, mask, n, vec, lamda, stats, gloss, gpred);
  return mode::check_launch(who);
}
