// Self-supervised stereo loss on rectified Cassini pairs (include/mode_hip.h): the right image warped to the left view along
// its rows by the predicted disparity, SSIM + L1 over 3x3 windows whose rows wrap (H is the periodic axis of a Cassini image), and an
// edge-aware smoothness term -- forward with a deterministic reduction, backward as a gather.
//
// One workgroup per 16 x 32 tile of one image and one disparity map (K on grid.y).  The tile and its halo are staged in LDS once for
// all three channels: the de-normalised left image L, the warped right image Rh, dn = d / W and the validity bits.  The right image is
// read through the disparity straight from global memory (x0 and x0 + 1 of the pixel's own row).  The forward needs the windows of the
// tile (halo 1); the backward the windows one pixel beyond it (halo 2): channel by channel, a second pass over LDS leaves the three
// coefficients of d ssim / d Rh of every such window next to its two means, and a pixel then collects the up to nine windows that
// contain it.
// Per-pixel arithmetic is fp32 and the same instruction sequence for every pixel, whatever its place in the tile: rolling the inputs
// along H rolls the gradient bit for bit.
//
// The reduction is the scheme of metrics_internal.h with four statistics per map: a thread walks its pixels in ascending order, a
// fixed butterfly, the waves in index order, one slab column per workgroup, and a second launch folds the columns in index order.
// No atomics; the same inputs give the same bits on any stream.
#include <math.h>

#include "common.h"
#include "mode_hip_selfsup.h"

namespace {

constexpr int NT = 256;  // threads per workgroup (4 waves)
constexpr int TH = 16;   // tile rows (along H, the periodic axis)
constexpr int TW = 32;   // tile columns (along W, contiguous in memory)
constexpr int kS = MODE_PHOTOMETRIC_STATS;
constexpr int kMaxK = MODE_PHOTOMETRIC_MAX_MAPS;

// Kernel-side copy of mode_photometric_params (by value: it travels in the kernel arguments).
struct Prm {
  float alpha, lam, beta, c1, c2;
  float mean[3], std[3];
  float wgt[kMaxK];
};

template <int HALO>
struct Stage {
  static constexpr int RH = TH + 2 * HALO, RW = TW + 2 * HALO, N = RH * RW;
  float L[3][N];   // left image, de-normalised
  float R[3][N];   // right image warped to the left view (0 where invalid)
  float dn[N];     // d / W
  unsigned char ok[N];
};

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }  // sign(0) = 0, sign(NaN) = 0

// The warp of one pixel: row = &right[b][0][h][0], HW the channel stride.  rh: the interpolated colour; slope: d rh / d d, which is
// R[x0] - R[x0 + 1] in the left view (VIEW 0: x = w - d) and R[x0 + 1] - R[x0] in the right view (VIEW 1: x = w + d; DESIGN 24, where
// "right" is the other camera's image, whichever that is).
template <int VIEW>
__device__ __forceinline__ bool warp_pixel(const float* __restrict__ row, int HW, int W, int w, float d, const Prm& p, float rh[3],
                                           float slope[3]) {
  const float x = VIEW == 0 ? (float)w - d : (float)w + d;
  const bool ok = __builtin_isfinite(d) && x >= 0.f && x <= (float)(W - 1);
  if (!ok) {
    rh[0] = rh[1] = rh[2] = 0.f;
    slope[0] = slope[1] = slope[2] = 0.f;
    return false;
  }
  int x0 = (int)floorf(x);
  x0 = x0 < W - 2 ? x0 : W - 2;
  const float t = x - (float)x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r0 = row[c * HW + x0] * p.std[c] + p.mean[c];
    const float r1 = row[c * HW + x0 + 1] * p.std[c] + p.mean[c];
    rh[c] = (1.f - t) * r0 + t * r1;
    slope[c] = VIEW == 0 ? r0 - r1 : r1 - r0;
  }
  return true;
}

// Tile (h0, w0) and its halo into LDS.  Rows wrap modulo H; columns outside [0, W) are invalid pixels with L = Rh = dn = 0 (no window
// that exists contains them: windows have 1 <= w <= W - 2).  left, right: the image of this batch element; disp: this map's plane.
// MASKED: a pixel whose byte in mask (this map's plane) is zero is invalid; its L, Rh and dn are staged as ever.
template <int HALO, int VIEW, bool MASKED>
__device__ __forceinline__ void stage_tile(Stage<HALO>& s, const float* __restrict__ left, const float* __restrict__ right,
                                           const float* __restrict__ disp, const unsigned char* __restrict__ mask, int H, int W, int h0,
                                           int w0, const Prm& p) {
  using S = Stage<HALO>;
  const int HW = H * W;
  const float wf = (float)W;
  for (int i = threadIdx.x; i < S::N; i += NT) {
    const int r = i / S::RW, c = i - r * S::RW;
    int h = (h0 - HALO + r) % H;
    h = h < 0 ? h + H : h;
    const int w = w0 - HALO + c;
    float l[3] = {0.f, 0.f, 0.f}, rh[3] = {0.f, 0.f, 0.f}, slope[3];
    float dn = 0.f;
    bool ok = false;
    if (w >= 0 && w < W) {
      const int off = h * W + w;
      const float d = disp[off];
      dn = d / wf;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) l[ch] = left[ch * HW + off] * p.std[ch] + p.mean[ch];
      ok = warp_pixel<VIEW>(right + h * W, HW, W, w, d, p, rh, slope);
      if (MASKED) ok = ok && mask[off] != 0;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      s.L[ch][i] = l[ch];
      s.R[ch][i] = rh[ch];
    }
    s.dn[i] = dn;
    s.ok[i] = ok ? 1 : 0;
  }
}

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

// exp(-beta mean_c |L_c(a) - L_c(b)|): the edge weight between two staged pixels
template <int N>
__device__ __forceinline__ float edge_weight(const float (*L)[N], int a, int b, float beta) {
  const float e = (fabsf(L[0][a] - L[0][b]) + fabsf(L[1][a] - L[1][b]) + fabsf(L[2][a] - L[2][b])) * (1.f / 3.f);
  return expf(-beta * e);
}

// The whole block (all NT threads call it): fixed butterfly over the lanes, the waves in index order, statistic j of map k into
// slab[(k * kS + j) * ncols + col].
__device__ __forceinline__ void block_fold(const double (&a)[kS], double (*sh)[kS], double* __restrict__ slab, int k, int ncols, int col) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kS; ++j) {
    double v = a[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kS) {
    const int j = threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v += sh[w][j];
    slab[((long long)k * kS + j) * ncols + col] = v;
  }
}

// grid = (B * tiles, K).  Block (col, k) leaves its four statistics in column col of map k's slab rows.
template <int VIEW, bool MASKED>
__global__ __launch_bounds__(NT) void photometric_fwd_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                             const float* __restrict__ disp, const unsigned char* __restrict__ mask, int B,
                                                             int H, int W, int tiles_w, int tiles, Prm p, double* __restrict__ slab) {
  using S = Stage<1>;
  __shared__ S s;
  __shared__ double sh[NT / 64][kS];
  const int col = blockIdx.x, k = blockIdx.y;
  const int b = col / tiles, t = col - b * tiles;
  const int h0 = (t / tiles_w) * TH, w0 = (t % tiles_w) * TW;
  const long long HW = (long long)H * W;
  const long long plane = HW * ((long long)k * B + b);
  stage_tile<1, VIEW, MASKED>(s, left + 3 * HW * b, right + 3 * HW * b, disp + plane, MASKED ? mask + plane : nullptr, H, W, h0, w0, p);
  __syncthreads();
  double acc[kS] = {0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < TH * TW; j += NT) {
    const int r = j / TW, c = j - r * TW;
    const int h = h0 + r, w = w0 + c;
    if (h >= H || w >= W) continue;
    const int i = (r + 1) * S::RW + (c + 1);
    const float dn = s.dn[i];
    if (w <= W - 2) acc[MODE_PHOTOMETRIC_SUM_SMOOTH_X] += (double)(fabsf(s.dn[i + 1] - dn) * edge_weight(s.L, i + 1, i, p.beta));
    acc[MODE_PHOTOMETRIC_SUM_SMOOTH_Y] += (double)(fabsf(s.dn[i + S::RW] - dn) * edge_weight(s.L, i + S::RW, i, p.beta));
    if (w >= 1 && w <= W - 2 && window_ok<S::RW>(s.ok, i)) {
      float pe = 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const Moments m = window_moments<S::RW>(s.L[ch], s.R[ch], i);
        const float ssim = (2.f * m.mx * m.my + p.c1) * (2.f * m.cxy + p.c2) / ((m.mx * m.mx + m.my * m.my + p.c1) * (m.vx + m.vy + p.c2));
        pe += p.alpha * (1.f - ssim) / 2.f + (1.f - p.alpha) * fabsf(s.L[ch][i] - s.R[ch][i]);
      }
      acc[MODE_PHOTOMETRIC_N_VALID] += 1.0;
      acc[MODE_PHOTOMETRIC_SUM_PE] += (double)(pe * (1.f / 3.f));
    }
  }
  block_fold(acc, sh, slab, k, gridDim.x, col);
}

// One block: fold the columns of every (map, statistic) row in index order (thread t takes columns t, t + NT, ...; then the fixed
// butterfly and wave order), write stats (K x kS) and loss = sum_k wgt[k] (photo_k + lam smooth_k).
__global__ __launch_bounds__(NT) void photometric_final_kernel(const double* __restrict__ slab, int ncols, int K, int B, int H, int W, Prm p,
                                                               double* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double sh[NT / 64][kMaxK * kS];
  __shared__ double fin[kMaxK * kS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // All rows side by side: a row's columns still arrive in ascending order, but the loads of the 16 rows are independent.  One row
  // after the other, this single block waited for 24 dependent loads per row at 12 x 1024 x 512 (146 us; 35 us this way).
  constexpr int kRows = kMaxK * kS;
  const int nrows = K * kS;
  double v[kRows];
#pragma unroll
  for (int row = 0; row < kRows; ++row) v[row] = 0.0;
  for (int c = threadIdx.x; c < ncols; c += NT) {
    double t[kRows];  // every load issued before the first sum; rows at and beyond nrows re-read row 0 and are never written out
#pragma unroll
    for (int row = 0; row < kRows; ++row) t[row] = slab[(long long)(row < nrows ? row : 0) * ncols + c];
#pragma unroll
    for (int row = 0; row < kRows; ++row) v[row] += t[row];
  }
#pragma unroll
  for (int row = 0; row < kRows; ++row) {
    double t = v[row];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) sh[wave][row] = t;
  }
  __syncthreads();
  if (threadIdx.x < K * kS) {
    const int row = threadIdx.x;
    double v = sh[0][row];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v += sh[w][row];
    stats[row] = v;
    fin[row] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* f = fin + k * kS;
      const double n = f[MODE_PHOTOMETRIC_N_VALID];
      double term = f[MODE_PHOTOMETRIC_SUM_PE] / (n > 1.0 ? n : 1.0);
      if (p.lam != 0.f)  // lam == 0 leaves the term out: a NaN disparity then costs its pixel and nothing else
        term += (double)p.lam * (f[MODE_PHOTOMETRIC_SUM_SMOOTH_X] / ((double)B * H * (W - 1)) + f[MODE_PHOTOMETRIC_SUM_SMOOTH_Y] / ((double)B * H * W));
      total += (double)p.wgt[k] * term;
    }
    loss[0] = (float)total;
  }
}

// d ssim / d Rh_i of a valid window = (P + Q (L_i - mx) - R (Rh_i - my)) / 9; the backward keeps P, Q, R scaled by the factor of the
// photometric term, -alpha / (2 x 3 x 9), next to the two means -- for ONE channel at a time: the three channels take turns in the
// same 12 KiB, which keeps the kernel at 33 KiB of LDS (four workgroups per CU; all three at once were 58 KiB and two).
struct Windows {
  static constexpr int RH = TH + 2, RW = TW + 2, N = RH * RW;
  static constexpr int PER_THREAD = (N + NT - 1) / NT;
  float P[N], Q[N], R[N], mx[N], my[N];
  unsigned char ok[N];
};

// grid = (B * tiles, K).  gdisp is written once per element.
template <int VIEW, bool MASKED>
__global__ __launch_bounds__(NT) void photometric_bwd_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                             const float* __restrict__ disp, const unsigned char* __restrict__ mask, int B,
                                                             int H, int W, int tiles_w, int tiles, Prm p, const double* __restrict__ stats,
                                                             const float* __restrict__ gloss, float* __restrict__ gdisp) {
  using S = Stage<2>;
  constexpr int PX = TH * TW / NT;  // pixels per thread
  __shared__ S s;
  __shared__ Windows win;
  const int col = blockIdx.x, k = blockIdx.y;
  const int b = col / tiles, t = col - b * tiles;
  const int h0 = (t / tiles_w) * TH, w0 = (t % tiles_w) * TW;
  const long long HW = (long long)H * W;
  const float* rimg = right + 3 * HW * b;
  const float* dmap = disp + HW * ((long long)k * B + b);
  stage_tile<2, VIEW, MASKED>(s, left + 3 * HW * b, rimg, dmap, MASKED ? mask + HW * ((long long)k * B + b) : nullptr, H, W, h0, w0, p);
  __syncthreads();

  // this thread's windows (centred on the tile and one pixel around it): which of them exist and are valid
  bool wok[Windows::PER_THREAD];
#pragma unroll
  for (int n = 0; n < Windows::PER_THREAD; ++n) {
    const int i = threadIdx.x + n * NT;
    wok[n] = false;
    if (i < Windows::N) {
      const int r = i / Windows::RW, c = i - r * Windows::RW;
      const int w = w0 - 1 + c;
      wok[n] = w >= 1 && w <= W - 2 && window_ok<S::RW>(s.ok, (r + 1) * S::RW + (c + 1));
      win.ok[i] = wok[n] ? 1 : 0;
    }
  }
  // this thread's pixels: the slope of the warp (d Rh / d d) and where the photometric gradient gathers
  bool live[PX], valid[PX];
  float slope[PX][3], gph[PX];
#pragma unroll
  for (int n = 0; n < PX; ++n) {
    const int j = threadIdx.x + n * NT;
    const int r = j / TW, c = j - r * TW;
    const int h = h0 + r, w = w0 + c;
    live[n] = h < H && w < W;
    valid[n] = live[n] && s.ok[(r + 2) * S::RW + (c + 2)] != 0;
    gph[n] = 0.f;
    slope[n][0] = slope[n][1] = slope[n][2] = 0.f;
    if (valid[n]) {
      float rh[3];
      warp_pixel<VIEW>(rimg + h * W, (int)HW, W, w, dmap[h * W + w], p, rh, slope[n]);
    }
  }

  const float scale = -p.alpha / 54.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int n = 0; n < Windows::PER_THREAD; ++n) {
      const int i = threadIdx.x + n * NT;
      if (i < Windows::N) {
        float P = 0.f, Q = 0.f, R = 0.f, mx = 0.f, my = 0.f;
        if (wok[n]) {
          const int r = i / Windows::RW, c = i - r * Windows::RW;
          const Moments m = window_moments<S::RW>(s.L[ch], s.R[ch], (r + 1) * S::RW + (c + 1));
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
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < PX; ++n) {
      if (!valid[n]) continue;
      const int j = threadIdx.x + n * NT;
      const int r = j / TW, c = j - r * TW;
      const int i = (r + 2) * S::RW + (c + 2);
      const int wc = (r + 1) * Windows::RW + (c + 1);
      const float x = s.L[ch][i], y = s.R[ch][i];
      float a = 0.f;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int q = wc + dy * Windows::RW + dx;
          a += win.P[q] + win.Q[q] * (x - win.mx[q]) - win.R[q] * (y - win.my[q]);
        }
      if (win.ok[wc]) a += (1.f - p.alpha) * (1.f / 3.f) * sgn(y - x);
      gph[n] += slope[n][ch] * a;
    }
    __syncthreads();  // the next channel overwrites the windows
  }

  const double n_valid = stats[k * kS + MODE_PHOTOMETRIC_N_VALID];
  const double gw = (double)gloss[0] * (double)p.wgt[k];
  const float c_photo = (float)(gw / (n_valid > 1.0 ? n_valid : 1.0));
  const float c_sx = (float)(gw * (double)p.lam / ((double)W * ((double)B * H * (W - 1))));
  const float c_sy = (float)(gw * (double)p.lam / ((double)W * ((double)B * H * W)));
#pragma unroll
  for (int n = 0; n < PX; ++n) {
    if (!live[n]) continue;
    const int j = threadIdx.x + n * NT;
    const int r = j / TW, c = j - r * TW;
    const int h = h0 + r, w = w0 + c;
    const int i = (r + 2) * S::RW + (c + 2);
    float g = gph[n] * c_photo;
    if (p.lam != 0.f) {
      const float dn = s.dn[i];
      float gx = 0.f;
      if (w <= W - 2) gx -= sgn(s.dn[i + 1] - dn) * edge_weight(s.L, i + 1, i, p.beta);
      if (w >= 1) gx += sgn(dn - s.dn[i - 1]) * edge_weight(s.L, i, i - 1, p.beta);
      const float gy = sgn(dn - s.dn[i - S::RW]) * edge_weight(s.L, i, i - S::RW, p.beta) -
                       sgn(s.dn[i + S::RW] - dn) * edge_weight(s.L, i + S::RW, i, p.beta);
      g += c_sx * gx + c_sy * gy;
    }
    gdisp[HW * ((long long)k * B + b) + h * W + w] = g;
  }
}

// The checks the two launching entries share; fills p and the tiling.
int check_common(const char* who, const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                 const mode_photometric_params* params, Prm& p, int& tiles_w, int& tiles) {
  MODE_REQUIRE(left && right && disp && params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(K >= 1 && K <= kMaxK, MODE_ERR_BAD_ARG, "%s: K = %d disparity maps (1 .. %d)", who, K, kMaxK);
  MODE_REQUIRE(B >= 1, MODE_ERR_BAD_ARG, "%s: bad batch size %d", who, B);
  MODE_REQUIRE(H >= 3 && W >= 3, MODE_ERR_BAD_ARG, "%s: %d x %d: H and W must be at least 3 (one 3x3 window)", who, H, W);
  // In-image offsets (3 H W), the workgroup index (B x tiles) and W as an exact float are 32-bit quantities; bases are 64-bit.
  MODE_REQUIRE(3ll * B * H * W < (1ll << 31) && W < (1 << 24), MODE_ERR_UNSUPPORTED,
               "%s: images of 3 x %d x %d x %d elements: 32-bit indices need 3 B H W < 2^31 (and W < 2^24)", who, B, H, W);
  p.alpha = params->alpha;
  p.lam = params->lam;
  p.beta = params->beta;
  p.c1 = params->c1;
  p.c2 = params->c2;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = params->mean[c];
    p.std[c] = params->std[c];
  }
  for (int k = 0; k < kMaxK; ++k) p.wgt[k] = k < K ? params->weights[k] : 0.f;
  tiles_w = mode::cdiv(W, TW);
  tiles = tiles_w * mode::cdiv(H, TH);
  return MODE_OK;
}

// The forward's two launches and the backward's one, for one (view, masked) form of the kernels.
template <int VIEW, bool MASKED>
void launch_fwd(const float* left, const float* right, const float* disp, const unsigned char* mask, int K, int B, int H, int W, int tiles_w,
                int tiles, const Prm& p, double* slab, double* stats, float* loss, hipStream_t st) {
  const int ncols = B * tiles;
  hipLaunchKernelGGL((photometric_fwd_kernel<VIEW, MASKED>), dim3(ncols, K), dim3(NT), 0, st, left, right, disp, mask, B, H, W, tiles_w, tiles,
                     p, slab);
  hipLaunchKernelGGL(photometric_final_kernel, dim3(1), dim3(NT), 0, st, slab, ncols, K, B, H, W, p, stats, loss);
}

template <int VIEW, bool MASKED>
void launch_bwd(const float* left, const float* right, const float* disp, const unsigned char* mask, int K, int B, int H, int W, int tiles_w,
                int tiles, const Prm& p, const double* stats, const float* gloss, float* gdisp, hipStream_t st) {
  hipLaunchKernelGGL((photometric_bwd_kernel<VIEW, MASKED>), dim3(B * tiles, K), dim3(NT), 0, st, left, right, disp, mask, B, H, W, tiles_w,
                     tiles, p, stats, gloss, gdisp);
}

}  // namespace

extern "C" size_t mode_photometric_loss_workspace_bytes(int K, int B, int H, int W) {
  if (K < 1 || K > kMaxK || B < 1 || H < 3 || W < 3 || 3ll * B * H * W >= (1ll << 31)) return 0;
  const size_t cols = (size_t)B * mode::cdiv(W, TW) * mode::cdiv(H, TH);
  return ((size_t)K * kS * cols * sizeof(double) + 15) / 16 * 16;
}

extern "C" int mode_photometric_loss_fwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                                         const mode_photometric_params* params, void* workspace, size_t workspace_bytes, double* stats,
                                         float* loss, mode_stream_t stream) {
  const char* who = "mode_photometric_loss_fwd";
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, left, right, disp, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(workspace && ((size_t)workspace & 7) == 0, MODE_ERR_WORKSPACE, "%s: workspace missing or not 8-byte aligned", who);
  MODE_REQUIRE(workspace_bytes >= mode_photometric_loss_workspace_bytes(K, B, H, W), MODE_ERR_WORKSPACE,
               "%s: workspace of %zu B is too small (needs %zu B)", who, workspace_bytes, mode_photometric_loss_workspace_bytes(K, B, H, W));
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  launch_fwd<0, false>(left, right, disp, nullptr, K, B, H, W, tiles_w, tiles, p, slab, stats, loss, st);
  return mode::check_launch(who);
}

extern "C" int mode_photometric_loss_bwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                                         const mode_photometric_params* params, const double* stats, const float* gloss, float* gdisp,
                                         mode_stream_t stream) {
  const char* who = "mode_photometric_loss_bwd";
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, left, right, disp, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && gloss && gdisp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  launch_bwd<0, false>(left, right, disp, nullptr, K, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp, mode::as_stream(stream));
  return mode::check_launch(who);
}

// ---------------------------------------------------------------------------------------------- either view, with a mask
// include/mode_hip_selfsup.h.  The same kernels with the view and the mask as template parameters; view 0 without a mask launches the
// instantiation of the entries above.
extern "C" int mode_selfsup_view_loss_fwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask,
                                          int view, int K, int B, int H, int W, const mode_photometric_params* params, void* workspace,
                                          size_t workspace_bytes, double* stats, float* loss, mode_stream_t stream) {
  const char* who = "mode_selfsup_view_loss_fwd";
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, own_image, other_image, disp, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(view == 0 || view == 1, MODE_ERR_BAD_ARG, "%s: view = %d (0: left, 1: right)", who, view);
  MODE_REQUIRE(stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(workspace && ((size_t)workspace & 7) == 0, MODE_ERR_WORKSPACE, "%s: workspace missing or not 8-byte aligned", who);
  MODE_REQUIRE(workspace_bytes >= mode_photometric_loss_workspace_bytes(K, B, H, W), MODE_ERR_WORKSPACE,
               "%s: workspace of %zu B is too small (needs %zu B)", who, workspace_bytes, mode_photometric_loss_workspace_bytes(K, B, H, W));
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  if (view == 0 && !mask) launch_fwd<0, false>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, slab, stats, loss, st);
  if (view == 0 && mask) launch_fwd<0, true>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, slab, stats, loss, st);
  if (view == 1 && !mask) launch_fwd<1, false>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, slab, stats, loss, st);
  if (view == 1 && mask) launch_fwd<1, true>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, slab, stats, loss, st);
  return mode::check_launch(who);
}

extern "C" int mode_selfsup_view_loss_bwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask,
                                          int view, int K, int B, int H, int W, const mode_photometric_params* params, const double* stats,
                                          const float* gloss, float* gdisp, mode_stream_t stream) {
  const char* who = "mode_selfsup_view_loss_bwd";
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, own_image, other_image, disp, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(view == 0 || view == 1, MODE_ERR_BAD_ARG, "%s: view = %d (0: left, 1: right)", who, view);
  MODE_REQUIRE(stats && gloss && gdisp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  hipStream_t st = mode::as_stream(stream);
  if (view == 0 && !mask) launch_bwd<0, false>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp, st);
  if (view == 0 && mask) launch_bwd<0, true>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp, st);
  if (view == 1 && !mask) launch_bwd<1, false>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp, st);
  if (view == 1 && mask) launch_bwd<1, true>(own_image, other_image, disp, mask, K, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp, st);
  return mode::check_launch(who);
}
