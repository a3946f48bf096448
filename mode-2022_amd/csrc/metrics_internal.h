// The deterministic masked reduction of the metric entries, shared by the flat-range entries (metrics.hip) and the per-frame
// panorama scoring (erp_metrics.hip).  Every piece here was moved out of metrics.hip unchanged, so whatever includes this header
// forms the old entries' bits.
//
// The scheme: element quad q (elements 4q .. 4q + 3) belongs to thread q % T of a grid of T = 256 * metric_blocks(n) threads that
// depends on n alone, every thread walks its quads in ascending order, a block reduces its threads by a fixed butterfly and a fixed
// wave order (block_fold), writes its partials to its own slab column, and a second launch folds the columns in index order
// (fold_columns).  No atomics; the same n gives the same bits on any stream, whatever the placement or arrival order of the blocks.
#pragma once
#include <math.h>

#include "common.h"

namespace mode {
namespace metrics {

constexpr int NT = 256;                              // threads per block (4 waves)
constexpr int kMaxBlocks = 1024;                     // grid cap of the streaming pass: 4 blocks per CU, grid-stride beyond
constexpr int kT = MODE_METRICS_MAX_THRESHOLDS;
constexpr int kS = MODE_METRICS_COUNT;               // statistics per slab row

inline int metric_blocks(long long n) {
  const long long quads = (n + 3) / 4;
  const long long b = (quads + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// Kernel-side copy of mode_metrics_params (by value: it travels in the kernel arguments).
struct Thresholds {
  int n_px, n_d1, n_ratio;
  float px[kT], d1_px[kT], d1_pct[kT], ratio[kT];
};

// params -> th on the host, with the count checks of every entry that takes thresholds
inline int load_thresholds(const mode_metrics_params* params, Thresholds& th, const char* who) {
  MODE_REQUIRE(params->n_px >= 0 && params->n_px <= kT && params->n_d1 >= 0 && params->n_d1 <= kT && params->n_ratio >= 0 &&
                   params->n_ratio <= kT,
               MODE_ERR_BAD_ARG, "%s: too many thresholds (at most %d of each kind)", who, kT);
  th.n_px = params->n_px;
  th.n_d1 = params->n_d1;
  th.n_ratio = params->n_ratio;
  for (int k = 0; k < kT; ++k) {
    th.px[k] = params->px[k];
    th.d1_px[k] = params->d1_px[k];
    th.d1_pct[k] = params->d1_pct[k];
    th.ratio[k] = params->ratio[k];
  }
  return MODE_OK;
}

#ifdef __HIPCC__
// torch.max / torch.maximum: NaN wins.  One canonical NaN, so that the reduced maximum has the same bits whichever NaN came first.
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }

struct Acc {
  unsigned n, n_gt, n_both;
  unsigned px[kT], d1[kT], ratio[kT];
  double s_abs, s_sq, s_absrel, s_sqrel, s_log, s_log2;
  float max_abs;
};

// One element, every term in fp32 exactly as the reference's torch expressions form it (IEEE division, the scalar thresholds
// rounded to fp32 as torch casts a Python scalar to the tensor's dtype), the logs in fp64.
template <bool kLogOnly>
__device__ __forceinline__ void accumulate(Acc& a, float p, float g, bool sel, const Thresholds& th) {
  if (!sel) return;
  if (!kLogOnly) {
    const float d = p - g;
    const float e = fabsf(d);
    const float d2 = d * d;
    a.n += 1;
    a.s_abs += (double)e;
    a.s_sq += (double)d2;
    a.max_abs = nan_max(a.max_abs, e);
#pragma unroll
    for (int k = 0; k < kT; ++k) {
      if (k < th.n_px) a.px[k] += (e >= th.px[k]) ? 1u : 0u;
      if (k < th.n_d1) {
        const float tg = th.d1_pct[k] * g;
        a.d1[k] += (e >= th.d1_px[k] && e >= tg) ? 1u : 0u;
      }
    }
    if (th.n_ratio > 0) {
      const float q = p / g, r = g / p;
      const float m = nan_max(q, r);
#pragma unroll
      for (int k = 0; k < kT; ++k)
        if (k < th.n_ratio) a.ratio[k] += (m < th.ratio[k]) ? 1u : 0u;
    }
    if (g > 0.f) {
      const float g2 = g * g;
      a.n_gt += 1;
      a.s_absrel += (double)(e / g);
      a.s_sqrel += (double)(d2 / g2);
    }
  }
  if (g > 0.f && p > 0.f) {
    const double l = log((double)p) - log((double)g);
    a.n_both += 1;
    a.s_log += l;
    a.s_log2 += l * l;
  }
}

// The statistic vector of one thread, in the order of include/mode_hip.h (all as fp64: counts are exact below 2^53).
__device__ __forceinline__ double stat_of(const Acc& a, int j) {
  switch (j) {
    case MODE_METRICS_N: return (double)a.n;
    case MODE_METRICS_N_GT: return (double)a.n_gt;
    case MODE_METRICS_N_BOTH: return (double)a.n_both;
    case MODE_METRICS_SUM_ABS: return a.s_abs;
    case MODE_METRICS_SUM_SQ: return a.s_sq;
    case MODE_METRICS_SUM_ABSREL: return a.s_absrel;
    case MODE_METRICS_SUM_SQREL: return a.s_sqrel;
    case MODE_METRICS_SUM_LOG: return a.s_log;
    case MODE_METRICS_SUM_LOG2: return a.s_log2;
    case MODE_METRICS_MAX_ABS: return (double)a.max_abs;
    default:
      if (j < MODE_METRICS_D1) return (double)a.px[j - MODE_METRICS_PX];
      if (j < MODE_METRICS_RATIO) return (double)a.d1[j - MODE_METRICS_D1];
      return (double)a.ratio[j - MODE_METRICS_RATIO];
  }
}

__device__ __forceinline__ double combine(int j, double a, double b) {
  if (j == MODE_METRICS_MAX_ABS) return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b);
  return a + b;
}

// Stage 1 tail, whole block (NT threads, all of them call it): the fixed butterfly over the lanes, the waves in index order, and the
// block's statistics into column `col` of a slab of `ncols` columns (slab[j * ncols + col]).  sh: NT / 64 rows of LDS.
__device__ __forceinline__ void block_fold(const Acc& a, double (*sh)[kS], double* __restrict__ slab, int ncols, int col) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kS; ++j) {
    double v = stat_of(a, j);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = combine(j, v, __shfl_xor(v, off, 64));
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kS) {
    const int j = threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v = combine(j, v, sh[w][j]);
    slab[(long long)j * ncols + col] = v;
  }
}

// Stage 2, one block per slab: fold the nblocks columns in index order (thread t takes columns t, t + NT, ...; then the fixed
// butterfly and wave order) and write the statistic vector to out and to fin (LDS, kS entries; valid after a __syncthreads()).
__device__ __forceinline__ void fold_columns(const double* __restrict__ slab, int nblocks, double (*sh)[kS], double* __restrict__ out,
                                             double* fin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kS; ++j) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += NT) v = combine(j, v, slab[(long long)j * nblocks + b]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = combine(j, v, __shfl_xor(v, off, 64));
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kS) {
    const int j = threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v = combine(j, v, sh[w][j]);
    out[j] = v;
    fin[j] = v;
  }
}
#endif  // __HIPCC__

}  // namespace metrics
}  // namespace mode
