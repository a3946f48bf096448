// What the photometric loss family shares: photometric.hip (stereo view loss), lr_consistency.hip (left-right consistency)
// and mv_photometric.hip (multi-view reprojection).  Every piece here was moved out of those files unchanged, and the standing rule
// for this header is that a kernel compiles to the same gfx950 code with a piece as it did with its own copy; DESIGN 26 names the
// three kernels that the two folds left with other scalar code.  The shape of some pieces follows from the rule: the loop over a
// pixel's nine windows and the SSIM formula of the forward stay with the caller, because the compiler optimises a helper before it
// inlines it, and a helper that holds them leaves the kernels with other code.
//
// The frame: one workgroup of NT threads per TH x TW tile, the tile and its halo staged in LDS by the including file (the staging is
// what differs between the losses and stays with them).  Here: the 3x3 windows on the staged planes (validity, moments, the
// SSIM + L1 term, the coefficients of d ssim / d R and what one window sends a pixel), the edge weight of the smoothness terms, and
// the deterministic reduction (the scheme of metrics_internal.h: a fixed butterfly, the waves in index order, one slab column per
// workgroup, a one-block fold of the columns in index order; no atomics).  On the host: the colour parameters and the checks that
// the entries of the family make with the same words.
#pragma once
#include <math.h>

#include "common.h"

namespace mode {
namespace photometric {

constexpr int NT = 256;  // threads per workgroup (4 waves)
constexpr int TH = 16;   // tile rows (along H, the periodic axis)
constexpr int TW = 32;   // tile columns (along W, contiguous in memory)

// The colour part of mode_photometric_params, kernel-side (by value: it travels in the kernel arguments).
struct Colour {
  float alpha, lam, beta, c1, c2;
  float mean[3], std[3];
};

inline void load_colour(const mode_photometric_params* params, Colour& p) {
  p.alpha = params->alpha;
  p.lam = params->lam;
  p.beta = params->beta;
  p.c1 = params->c1;
  p.c2 = params->c2;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = params->mean[c];
    p.std[c] = params->std[c];
  }
}

// Tiles of one H x W image: the slab of a tiled forward has one column per tile and image.
inline size_t tiles_of(int H, int W) { return (size_t)mode::cdiv(W, TW) * mode::cdiv(H, TH); }

// One 3x3 window needs H, W >= 3; fills the tiling.
inline int check_tiling(const char* who, int H, int W, int& tiles_w, int& tiles) {
  MODE_REQUIRE(H >= 3 && W >= 3, MODE_ERR_BAD_ARG, "%s: %d x %d: H and W must be at least 3 (one 3x3 window)", who, H, W);
  tiles_w = mode::cdiv(W, TW);
  tiles = tiles_w * mode::cdiv(H, TH);
  return MODE_OK;
}

// The slab of a forward entry: `need` is what its workspace_bytes function answers for the call's shape.
inline int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  MODE_REQUIRE(workspace && ((size_t)workspace & 7) == 0, MODE_ERR_WORKSPACE, "%s: workspace missing or not 8-byte aligned", who);
  MODE_REQUIRE(workspace_bytes >= need, MODE_ERR_WORKSPACE, "%s: workspace of %zu B is too small (needs %zu B)", who, workspace_bytes, need);
  return MODE_OK;
}

#ifdef __HIPCC__
__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }  // sign(0) = 0, sign(NaN) = 0

// RW: the row pitch of the staged planes; centre: the window's centre in them.
template <int RW>
__device__ __forceinline__ bool window_ok(const unsigned char* ok, int centre) {
  unsigned v = 1;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) v &= ok[centre + dy * RW + dx];
  return v != 0;
}

// The centred, biased moments of one window and channel, every sum in the order dy = -1..1, dx = -1..1.
struct Moments {
  float mx, my, vx, vy, cxy;
};

template <int RW>
__device__ __forceinline__ Moments window_moments(const float* __restrict__ L, const float* __restrict__ R, int centre) {
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      sx += L[centre + dy * RW + dx];
      sy += R[centre + dy * RW + dx];
    }
  Moments m;
  constexpr float k9 = 1.f / 9.f;  // (a multiplication: an IEEE division costs a dozen instructions, and the windows have ten)
  m.mx = sx * k9;
  m.my = sy * k9;
  float vx = 0.f, vy = 0.f, cxy = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float a = L[centre + dy * RW + dx] - m.mx, b = R[centre + dy * RW + dx] - m.my;
      vx += a * a;
      vy += b * b;
      cxy += a * b;
    }
  m.vx = vx * k9;
  m.vy = vy * k9;
  m.cxy = cxy * k9;
  return m;
}

// One channel's photometric term of a window from its SSIM and the centre's two values.  (The forward kernels form
// ssim = (2 mx my + c1)(2 cxy + c2) / ((mx^2 + my^2 + c1)(vx + vy + c2)) from the moments themselves, in one line: as a helper of this
// header that line leaves mvphoto_fwd_kernel with other code.)
__device__ __forceinline__ float window_term(float ssim, float l, float r, float alpha) {
  return alpha * (1.f - ssim) / 2.f + (1.f - alpha) * fabsf(l - r);
}

// exp(-beta mean_c |L_c(a) - L_c(b)|): the edge weight between two staged pixels
template <int N>
__device__ __forceinline__ float edge_weight(const float (*L)[N], int a, int b, float beta) {
  const float e = (fabsf(L[0][a] - L[0][b]) + fabsf(L[1][a] - L[1][b]) + fabsf(L[2][a] - L[2][b])) * (1.f / 3.f);
  return expf(-beta * e);
}

// d ssim / d R_i of a window = (P + Q (L_i - mx) - R (R_i - my)) / 9; the backward keeps P, Q, R scaled by the factor of the
// photometric term, -alpha / (2 x 3 x 9), next to the two means -- for ONE channel at a time: the three channels take turns in the
// same 12 KiB (photometric.hip stays at 33 KiB of LDS and four workgroups per CU; all three at once were 58 KiB and two).  The windows
// are those centred on the tile and one pixel around it; tag: one byte per window that does not change with the channel (whether it
// is valid; the source that won it).
struct Windows {
  static constexpr int RH = TH + 2, RW = TW + 2, N = RH * RW;
  static constexpr int PER_THREAD = (N + NT - 1) / NT;
  float P[N], Q[N], R[N], mx[N], my[N];
  unsigned char tag[N];
};

__device__ __forceinline__ float window_scale(const Colour& p) { return -p.alpha / 54.f; }

// Window i of one channel into win: its coefficients if it is `live`, zeros if not.  L, R: that channel's planes, staged with halo 2
// and row pitch SRW; scale: window_scale.
template <int SRW>
__device__ __forceinline__ void put_window(Windows& win, int i, bool live, const float* L, const float* R_, float scale, const Colour& p) {
  float P = 0.f, Q = 0.f, R = 0.f, mx = 0.f, my = 0.f;
  if (live) {
    const int r = i / Windows::RW, c = i - r * Windows::RW;
    const Moments m = window_moments<SRW>(L, R_, (r + 1) * SRW + (c + 1));
    const float a1 = 2.f * m.mx * m.my + p.c1, a2 = 2.f * m.cxy + p.c2;
    const float b1 = m.mx * m.mx + m.my * m.my + p.c1, b2 = m.vx + m.vy + p.c2;
    const float r1 = 1.f / b1, r2 = 1.f / b2;
    const float inv = r1 * r2;
    const float ssim = a1 * a2 * inv;
    P = scale * 2.f * (m.mx * a2 * inv - ssim * m.my * r1);
    Q = scale * 2.f * a1 * inv;
    R = scale * 2.f * ssim * r2;
    mx = m.mx;
    my = m.my;
  }
  win.P[i] = P;
  win.Q[i] = Q;
  win.R[i] = R;
  win.mx[i] = mx;
  win.my[i] = my;
}

// What window q sends a pixel it contains, x and y the pixel's two values; a pixel adds its nine windows in the order dy = -1..1,
// dx = -1..1.
__device__ __forceinline__ float window_share(const Windows& win, int q, float x, float y) {
  return win.P[q] + win.Q[q] * (x - win.mx[q]) - win.R[q] * (y - win.my[q]);
}

// Stage 1 tail, whole block (all NTB threads call it): the fixed butterfly over the lanes, the waves in index order, and statistic j
// of the block into slab[row_of(j) * ncols + col] (row_of: int -> long long).  sh: NTB / 64 rows of LDS.
template <int KS, int NTB, typename RowOf>
__device__ __forceinline__ void block_fold(const double (&a)[KS], double (*sh)[KS], double* __restrict__ slab, RowOf row_of, int ncols,
                                           int col) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    double v = a[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < KS) {
    const int j = threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int w = 1; w < NTB / 64; ++w) v += sh[w][j];
    slab[row_of(j) * ncols + col] = v;
  }
}

// Stage 2, one block of NTB threads: fold the columns of the first nrows (<= ROWS) slab rows in index order (thread t takes columns
// t, t + NTB, ...; then the fixed butterfly and wave order) and write the totals to stats and to fin (LDS; valid after a
// __syncthreads()), from where the caller forms its loss.  All rows side by side: a row's columns still arrive in ascending order,
// but the loads of the rows are independent.  One row after the other, this single block waited for 24 dependent loads per row at
// 12 x 1024 x 512 (146 us; 35 us this way).  sh: NTB / 64 rows of LDS.
template <int ROWS, int NTB>
__device__ __forceinline__ void fold_rows(const double* slab, int ncols, int nrows, double (*sh)[ROWS], double* stats, double* fin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double v[ROWS];
#pragma unroll
  for (int row = 0; row < ROWS; ++row) v[row] = 0.0;
  for (int c = threadIdx.x; c < ncols; c += NTB) {
    double t[ROWS];  // every load issued before the first sum; rows at and beyond nrows re-read row 0 and are never written out
#pragma unroll
    for (int row = 0; row < ROWS; ++row) t[row] = slab[(long long)(row < nrows ? row : 0) * ncols + c];
#pragma unroll
    for (int row = 0; row < ROWS; ++row) v[row] += t[row];
  }
#pragma unroll
  for (int row = 0; row < ROWS; ++row) {
    double t = v[row];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) sh[wave][row] = t;
  }
  __syncthreads();
  if (threadIdx.x < nrows) {
    const int row = threadIdx.x;
    double t = sh[0][row];
#pragma unroll
    for (int w = 1; w < NTB / 64; ++w) t += sh[w][row];
    stats[row] = t;
    fin[row] = t;
  }
}
#endif  // __HIPCC__

}  // namespace photometric
}  // namespace mode
