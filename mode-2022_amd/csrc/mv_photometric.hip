// Multi-view reprojection loss of a fused depth map (include/mode_hip_mvphoto.h): every pixel of the reference panorama is
// lifted by its depth, projected into S other panoramas of known pose and sampled there (bilinear, rows wrap); SSIM + L1 over 3x3
// windows between the reference and each warped source, the per-window minimum over the sources, and an edge-aware smoothness term
// on log depth -- forward with a deterministic reduction, backward as a gather.
//
// The frame is that of photometric_internal.h: one workgroup per 16 x 32 tile of one frame, the tile and its halo staged in LDS once
// for all three channels, the window arithmetic and the reduction from there.  What is here is this loss's own: the fp64 projection
// and its staging, the minimum over the sources, the smoothness on log depth, and the entries.
// The de-normalised reference L, log depth and its validity are staged once; the source loop runs inside the kernel: for each source the warped image Ih_s and its validity byte go into the same LDS planes (four global gathers per pixel and channel),
// pe_s is formed per window, and the running minimum and its index stay in registers.  A thread stages the same pixels for every
// source, so their viewing directions (fp64 sin / cos) are computed once and kept in registers.
// The geometry -- u, v and their slopes in depth -- is fp64, in one function that both passes call, and is rounded to fp32 at t, q
// and the slopes; validity and floor are discontinuous, and in fp64 the kernel and a float64 restatement agree on them.  Everything
// after is fp32 and the same instruction sequence for every pixel, whatever its place in the tile.
//
// The backward reads the forward's win: for each source it forms the three coefficients of d ssim / d Ih of the windows that source
// won, channel by channel in the same 12 KiB, and a pixel collects the up to nine windows that contain it, times the slope of source
// s at that pixel.  gdepth accumulates over the sources in registers and is written once per element.
//
// The reduction is the scheme of metrics_internal.h with twelve statistics: a thread walks its pixels in ascending order, a fixed
// butterfly, the waves in index order, one slab column per workgroup, and a second launch folds the columns in index order.
// No atomics; the same inputs give the same bits on any stream.
#include "mode_hip_mvphoto.h"
#include "photometric_internal.h"

static_assert(MODE_MVP_STATS == MODE_MVP_WINS + MODE_MVP_MAX_SOURCES, "one win count per source after the four sums");
static_assert(MODE_MVP_NO_WINNER >= MODE_MVP_MAX_SOURCES && MODE_MVP_NO_WINNER <= 255, "win is a byte");

namespace {

using namespace mode::photometric;

constexpr int PX = TH * TW / NT;  // tile pixels per thread
constexpr int kS = MODE_MVP_STATS;
constexpr int kMaxS = MODE_MVP_MAX_SOURCES;
constexpr int kNone = MODE_MVP_NO_WINNER;
constexpr double kPi = 3.14159265358979323846;

// Kernel-side copies of the parameters and of the poses (by value: they travel in the kernel arguments).
using Prm = Colour;

struct Poses {
  double p[kMaxS][12];  // [A | o], row-major 3 x 4
};

template <int HALO>
struct Stage {
  static constexpr int RH = TH + 2 * HALO, RW = TW + 2 * HALO, N = RH * RW;
  static constexpr int PER_THREAD = (N + NT - 1) / NT;
  float L[3][N];   // reference image, de-normalised
  float R[3][N];   // the current source warped to the reference view (0 where invalid)
  float ld[N];     // log depth (0 where the depth is not finite and > 0)
  unsigned char ok[N];   // valid for the current source
  unsigned char dok[N];  // depth finite and > 0
};

struct Dir {
  double x, y, z;
};

// The viewing direction of pixel (h, w), angles at the pixel's centre.
__device__ __forceinline__ Dir pixel_dir(int h, int w, int H, int W) {
  const double theta = kPi - ((double)h + 0.5) * 2.0 * kPi / (double)H;
  const double phi = kPi / 2 - ((double)w + 0.5) * kPi / (double)W;
  double st, ct, sp, cp;
  sincos(theta, &st, &ct);
  sincos(phi, &sp, &cp);
  Dir n;
  n.x = sp;
  n.y = cp * st;
  n.z = cp * ct;
  return n;
}

// Where one pixel lands in one source and how that moves with its depth.
struct Geo {
  int x0, ya, yb;  // columns x0, x0 + 1 (0 <= x0 <= W - 2); rows ya = y0 mod H, yb = (y0 + 1) mod H
  float t, q;      // u - x0, v - y0
  float du, dv;    // du / dD, dv / dD (SLOPES only)
};

// THE geometry, fp64, for forward and backward alike: depth D along n, pose P = [A | o] -> whether the pixel is valid for the source
// and, if so, g.  Rounded to fp32 only at t, q, du, dv.
template <bool SLOPES>
__device__ __forceinline__ bool project(float depth, const Dir& n, const double* __restrict__ P, int H, int W, Geo& g) {
  if (!(__builtin_isfinite(depth) && depth > 0.f)) return false;
  const double D = (double)depth;
  const double mx = P[0] * n.x + P[1] * n.y + P[2] * n.z;
  const double my = P[4] * n.x + P[5] * n.y + P[6] * n.z;
  const double mz = P[8] * n.x + P[9] * n.y + P[10] * n.z;
  const double Yx = D * mx + P[3], Yy = D * my + P[7], Yz = D * mz + P[11];
  const double s2 = Yy * Yy + Yz * Yz;
  const double r2 = Yx * Yx + s2;
  const double rho = sqrt(r2);
  if (!(rho > 0.0)) return false;
  const double phi = asin(Yx / rho);
  const double theta = atan2(Yy, Yz);
  const double u = (kPi / 2 - phi) * (double)W / kPi - 0.5;
  const double v = (kPi - theta) * (double)H / (2.0 * kPi) - 0.5;
  if (!(u >= 0.0 && u <= (double)(W - 1)) || !(v == v)) return false;  // pole to pole; this keeps the source's poles out as well
  const double fu = floor(u), fv = floor(v);
  int x0 = (int)fu;
  x0 = x0 < W - 2 ? x0 : W - 2;
  const int y0 = (int)fv;  // -1 .. H - 1
  g.x0 = x0;
  g.ya = ((y0 % H) + H) % H;
  g.yb = g.ya + 1 == H ? 0 : g.ya + 1;
  g.t = (float)(u - (double)x0);
  g.q = (float)(v - fv);
  if (SLOPES) {
    const double Ym = Yx * mx + Yy * my + Yz * mz;
    const double dphi = (mx * r2 - Yx * Ym) / (r2 * sqrt(s2));
    const double dtheta = (my * Yz - mz * Yy) / s2;
    g.du = (float)(-((double)W / kPi) * dphi);
    g.dv = (float)(-((double)H / (2.0 * kPi)) * dtheta);
  }
  return true;
}

// The bilinear value of the de-normalised source at g, and (SLOPES) d Ih / dD.  img: the three planes of one source of one frame.
template <bool SLOPES>
__device__ __forceinline__ void sample(const float* __restrict__ img, int HW, int W, const Geo& g, const Prm& p, float ih[3], float slope[3]) {
  const int a = g.ya * W + g.x0, b = g.yb * W + g.x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pl = img + c * HW;
    const float r00 = pl[a] * p.std[c] + p.mean[c], r01 = pl[a + 1] * p.std[c] + p.mean[c];
    const float r10 = pl[b] * p.std[c] + p.mean[c], r11 = pl[b + 1] * p.std[c] + p.mean[c];
    const float top = (1.f - g.t) * r00 + g.t * r01, bot = (1.f - g.t) * r10 + g.t * r11;
    ih[c] = (1.f - g.q) * top + g.q * bot;
    if (SLOPES) slope[c] = ((1.f - g.q) * (r01 - r00) + g.q * (r11 - r10)) * g.du + (bot - top) * g.dv;
  }
}

// What does not depend on the source, for tile (h0, w0) and its halo: L, log depth and its validity into LDS; the viewing direction
// and the depth of this thread's staged pixels into registers (dep = NaN for the columns outside [0, W): invalid for every source).
// Rows wrap modulo H; columns outside [0, W) are invalid pixels with L = 0 (no window that exists contains them).
template <int HALO>
__device__ __forceinline__ void stage_ref(Stage<HALO>& s, const float* __restrict__ ref, const float* __restrict__ depth, int H, int W,
                                          int h0, int w0, const Prm& p, Dir (&n)[Stage<HALO>::PER_THREAD], float (&dep)[Stage<HALO>::PER_THREAD]) {
  using S = Stage<HALO>;
  const int HW = H * W;
#pragma unroll
  for (int k = 0; k < S::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    dep[k] = __builtin_nanf("");
    n[k].x = n[k].y = n[k].z = 0.0;
    if (i >= S::N) continue;
    const int r = i / S::RW, c = i - r * S::RW;
    int h = (h0 - HALO + r) % H;
    h = h < 0 ? h + H : h;
    const int w = w0 - HALO + c;
    float l[3] = {0.f, 0.f, 0.f};
    float ld = 0.f;
    bool dok = false;
    if (w >= 0 && w < W) {
      const int off = h * W + w;
      const float d = depth[off];
      dep[k] = d;
      dok = __builtin_isfinite(d) && d > 0.f;
      ld = dok ? logf(d) : 0.f;
      n[k] = pixel_dir(h, w, H, W);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) l[ch] = ref[ch * HW + off] * p.std[ch] + p.mean[ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.L[ch][i] = l[ch];
    s.ld[i] = ld;
    s.dok[i] = dok ? 1 : 0;
  }
}

// One source warped into the R planes.  img: the three planes of that source of this frame; P: its pose.  SLOPES: d Ih / dD of the
// tile's own pixels (not the halo's) into slope[ch][r * TW + c].
template <int HALO, bool SLOPES>
__device__ __forceinline__ void stage_src(Stage<HALO>& s, const float* __restrict__ img, const double* __restrict__ P, int H, int W,
                                          const Prm& p, const Dir (&n)[Stage<HALO>::PER_THREAD], const float (&dep)[Stage<HALO>::PER_THREAD],
                                          float (*slope)[TH * TW]) {
  using S = Stage<HALO>;
#pragma unroll
  for (int k = 0; k < S::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    if (i >= S::N) continue;
    Geo g;
    float ih[3] = {0.f, 0.f, 0.f}, sl[3] = {0.f, 0.f, 0.f};
    const bool ok = project<SLOPES>(dep[k], n[k], P, H, W, g);
    if (ok) sample<SLOPES>(img, H * W, W, g, p, ih, sl);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.R[ch][i] = ih[ch];
    s.ok[i] = ok ? 1 : 0;
    if (SLOPES) {
      const int r = i / S::RW - HALO, c = i % S::RW - HALO;
      if (r >= 0 && r < TH && c >= 0 && c < TW) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) slope[ch][r * TW + c] = sl[ch];
      }
    }
  }
}

// grid = F * tiles.  Block col leaves its twelve statistics in column col of the slab and the winners of its tile in win.
__global__ __launch_bounds__(NT) void mvphoto_fwd_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                         const float* __restrict__ depth, Poses poses, int S, int H, int W, int tiles_w,
                                                         int tiles, Prm p, unsigned char* __restrict__ win, double* __restrict__ slab) {
  using St = Stage<1>;
  __shared__ St s;
  __shared__ double sh[NT / 64][kS];
  const int col = blockIdx.x;
  const int f = col / tiles, t = col - f * tiles;
  const int h0 = (t / tiles_w) * TH, w0 = (t % tiles_w) * TW;
  const long long HW = (long long)H * W;
  Dir n[St::PER_THREAD];
  float dep[St::PER_THREAD];
  stage_ref<1>(s, ref + 3 * HW * f, depth + HW * f, H, W, h0, w0, p, n, dep);

  float best[PX];
  int idx[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    best[k] = 0.f;
    idx[k] = kNone;
  }
  for (int sv = 0; sv < S; ++sv) {
    if (sv > 0) __syncthreads();  // every window of the previous source has been read
    stage_src<1, false>(s, src + 3 * HW * ((long long)f * S + sv), poses.p[sv], H, W, p, n, dep, nullptr);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int j = threadIdx.x + k * NT;
      const int r = j / TW, c = j - r * TW;
      const int h = h0 + r, w = w0 + c;
      if (h >= H || w < 1 || w > W - 2) continue;
      const int i = (r + 1) * St::RW + (c + 1);
      if (!window_ok<St::RW>(s.ok, i)) continue;
      float pe = 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const Moments m = window_moments<St::RW>(s.L[ch], s.R[ch], i);
        const float ssim = (2.f * m.mx * m.my + p.c1) * (2.f * m.cxy + p.c2) / ((m.mx * m.mx + m.my * m.my + p.c1) * (m.vx + m.vy + p.c2));
        pe += window_term(ssim, s.L[ch][i], s.R[ch][i], p.alpha);
      }
      pe *= 1.f / 3.f;
      if (idx[k] == kNone || pe < best[k]) {  // ascending s and a strict comparison: the smallest s that attains the minimum
        best[k] = pe;
        idx[k] = sv;
      }
    }
  }

  double acc[kS];
#pragma unroll
  for (int j = 0; j < kS; ++j) acc[j] = 0.0;
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int j = threadIdx.x + k * NT;
    const int r = j / TW, c = j - r * TW;
    const int h = h0 + r, w = w0 + c;
    if (h >= H || w >= W) continue;
    const int i = (r + 1) * St::RW + (c + 1);
    win[HW * f + h * W + w] = (unsigned char)idx[k];
    if (idx[k] != kNone) {
      acc[MODE_MVP_N] += 1.0;
      acc[MODE_MVP_SUM_MIN] += (double)best[k];
#pragma unroll
      for (int q = 0; q < kMaxS; ++q) acc[MODE_MVP_WINS + q] += idx[k] == q ? 1.0 : 0.0;
    }
    if (s.dok[i]) {
      const float ld = s.ld[i];
      if (w <= W - 2 && s.dok[i + 1]) acc[MODE_MVP_SUM_SMOOTH_X] += (double)(fabsf(s.ld[i + 1] - ld) * edge_weight(s.L, i + 1, i, p.beta));
      if (s.dok[i + St::RW]) acc[MODE_MVP_SUM_SMOOTH_Y] += (double)(fabsf(s.ld[i + St::RW] - ld) * edge_weight(s.L, i + St::RW, i, p.beta));
    }
  }
  block_fold<kS, NT>(acc, sh, slab, [](int j) { return (long long)j; }, gridDim.x, col);
}

// One block: fold the columns of every statistic in index order (thread t takes columns t, t + NT, ...; then the fixed butterfly and
// wave order), write stats and loss = photo + lam smooth.
__global__ __launch_bounds__(NT) void mvphoto_final_kernel(const double* __restrict__ slab, int ncols, int F, int H, int W, Prm p,
                                                           double* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double sh[NT / 64][kS];
  __shared__ double fin[kS];
  fold_rows<kS, NT>(slab, ncols, kS, sh, stats, fin);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = fin[MODE_MVP_N];
    double total = fin[MODE_MVP_SUM_MIN] / (n > 1.0 ? n : 1.0);
    if (p.lam != 0.f)  // lam == 0 leaves the term out
      total += (double)p.lam * (fin[MODE_MVP_SUM_SMOOTH_X] / ((double)F * H * (W - 1)) + fin[MODE_MVP_SUM_SMOOTH_Y] / ((double)F * H * W));
    loss[0] = (float)total;
  }
}

// grid = F * tiles.  gdepth is written once per element.
__global__ __launch_bounds__(NT) void mvphoto_bwd_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                         const float* __restrict__ depth, Poses poses, int S, int F, int H, int W,
                                                         int tiles_w, int tiles, Prm p, const unsigned char* __restrict__ win,
                                                         const double* __restrict__ stats, const float* __restrict__ gloss,
                                                         float* __restrict__ gdepth) {
  using St = Stage<2>;
  __shared__ St s;
  __shared__ Windows wn;
  __shared__ float slope[3][TH * TW];
  const int col = blockIdx.x;
  const int f = col / tiles, t = col - f * tiles;
  const int h0 = (t / tiles_w) * TH, w0 = (t % tiles_w) * TW;
  const long long HW = (long long)H * W;
  Dir n[St::PER_THREAD];
  float dep[St::PER_THREAD];
  stage_ref<2>(s, ref + 3 * HW * f, depth + HW * f, H, W, h0, w0, p, n, dep);
  // the winners of this thread's windows; columns outside 1 .. W - 2 have no window
  int mine[Windows::PER_THREAD];
#pragma unroll
  for (int k = 0; k < Windows::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    mine[k] = kNone;
    if (i < Windows::N) {
      const int r = i / Windows::RW, c = i - r * Windows::RW;
      int h = (h0 - 1 + r) % H;
      h = h < 0 ? h + H : h;
      const int w = w0 - 1 + c;
      if (w >= 1 && w <= W - 2) mine[k] = win[HW * f + h * W + w];
      wn.tag[i] = (unsigned char)mine[k];
    }
  }

  float gph[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) gph[k] = 0.f;
  const float scale = window_scale(p);
  for (int sv = 0; sv < S; ++sv) {
    int any = 0;
#pragma unroll
    for (int k = 0; k < Windows::PER_THREAD; ++k) any |= mine[k] == sv;
    if (!__syncthreads_or(any)) continue;  // (the barrier: the previous source's planes have been read.)  No window here is s's
    stage_src<2, true>(s, src + 3 * HW * ((long long)f * S + sv), poses.p[sv], H, W, p, n, dep, slope);
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int k = 0; k < Windows::PER_THREAD; ++k) {
        const int i = threadIdx.x + k * NT;
        if (i < Windows::N) put_window<St::RW>(wn, i, mine[k] == sv, s.L[ch], s.R[ch], scale, p);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        const int j = threadIdx.x + k * NT;
        const int r = j / TW, c = j - r * TW;
        const int i = (r + 2) * St::RW + (c + 2);
        const int wc = (r + 1) * Windows::RW + (c + 1);
        const float x = s.L[ch][i], y = s.R[ch][i];
        float a = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) a += window_share(wn, wc + dy * Windows::RW + dx, x, y);
        if (wn.tag[wc] == sv) a += (1.f - p.alpha) * (1.f / 3.f) * sgn(y - x);
        gph[k] += slope[ch][j] * a;  // (the slope is 0 where the pixel is invalid for s; no window of s contains such a pixel)
      }
      __syncthreads();  // the next channel overwrites the windows
    }
  }

  const double n_valid = stats[MODE_MVP_N];
  const double gw = (double)gloss[0];
  const float c_photo = (float)(gw / (n_valid > 1.0 ? n_valid : 1.0));
  const float c_sx = (float)(gw * (double)p.lam / ((double)F * H * (W - 1)));
  const float c_sy = (float)(gw * (double)p.lam / ((double)F * H * W));
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int j = threadIdx.x + k * NT;
    const int r = j / TW, c = j - r * TW;
    const int h = h0 + r, w = w0 + c;
    if (h >= H || w >= W) continue;
    const int i = (r + 2) * St::RW + (c + 2);
    float g = 0.f;
    if (s.dok[i]) {  // (a depth that is not finite and > 0 is invalid for every source and in no smoothness pair)
      g = gph[k] * c_photo;
      if (p.lam != 0.f) {
        const float ld = s.ld[i];
        float gx = 0.f, gy = 0.f;
        if (w <= W - 2 && s.dok[i + 1]) gx -= sgn(s.ld[i + 1] - ld) * edge_weight(s.L, i + 1, i, p.beta);
        if (w >= 1 && s.dok[i - 1]) gx += sgn(ld - s.ld[i - 1]) * edge_weight(s.L, i, i - 1, p.beta);
        if (s.dok[i - St::RW]) gy += sgn(ld - s.ld[i - St::RW]) * edge_weight(s.L, i, i - St::RW, p.beta);
        if (s.dok[i + St::RW]) gy -= sgn(s.ld[i + St::RW] - ld) * edge_weight(s.L, i + St::RW, i, p.beta);
        g += (c_sx * gx + c_sy * gy) / depth[HW * f + h * W + w];
      }
    }
    gdepth[HW * f + h * W + w] = g;
  }
}

// The checks the two launching entries share; fills p, the poses and the tiling.
int check_common(const char* who, const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                 const mode_photometric_params* params, Prm& p, Poses& ps, int& tiles_w, int& tiles) {
  MODE_REQUIRE(ref && src && depth && poses && params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(S >= 1 && S <= kMaxS, MODE_ERR_BAD_ARG, "%s: S = %d source views (1 .. %d)", who, S, kMaxS);
  MODE_REQUIRE(F >= 1, MODE_ERR_BAD_ARG, "%s: bad number of frames %d", who, F);
  int rc = check_tiling(who, H, W, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  for (int s = 0; s < kMaxS; ++s)
    for (int k = 0; k < 12; ++k) ps.p[s][k] = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* P = poses + 12 * s;
    for (int k = 0; k < 12; ++k) MODE_REQUIRE(std::isfinite(P[k]), MODE_ERR_BAD_ARG, "%s: pose %d, entry %d is not finite", who, s, k);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double dot = P[4 * a] * P[4 * b] + P[4 * a + 1] * P[4 * b + 1] + P[4 * a + 2] * P[4 * b + 2];
        MODE_REQUIRE(fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-9, MODE_ERR_BAD_ARG,
                     "%s: pose %d: A is not orthonormal to 1e-9 (row %d . row %d = %.17g)", who, s, a, b, dot);
      }
    for (int k = 0; k < 12; ++k) ps.p[s][k] = P[k];
  }
  // Offsets into the sources of one call (3 F S H W) and the workgroup index (F x tiles) are 32-bit quantities; bases are 64-bit.
  MODE_REQUIRE(3ll * F * S * H * W < (1ll << 31), MODE_ERR_UNSUPPORTED,
               "%s: sources of 3 x %d x %d x %d x %d elements: 32-bit indices need 3 F S H W < 2^31", who, F, S, H, W);
  load_colour(params, p);
  return MODE_OK;
}

}  // namespace

extern "C" int mode_mvphoto_version(void) { return MODE_MVPHOTO_VERSION; }

extern "C" size_t mode_mvphoto_workspace_bytes(int S, int F, int H, int W) {
  if (S < 1 || S > kMaxS || F < 1 || H < 3 || W < 3 || 3ll * F * S * H * W >= (1ll << 31)) return 0;
  return ((size_t)kS * F * tiles_of(H, W) * sizeof(double) + 15) / 16 * 16;
}

extern "C" int mode_mvphoto_loss_fwd(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                                     const mode_photometric_params* params, void* workspace, size_t workspace_bytes, unsigned char* win,
                                     double* stats, float* loss, mode_stream_t stream) {
  const char* who = "mode_mvphoto_loss_fwd";
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  MODE_REQUIRE(win && stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  int rc = check_common(who, ref, src, depth, poses, S, F, H, W, params, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  rc = check_workspace(who, workspace, workspace_bytes, mode_mvphoto_workspace_bytes(S, F, H, W));
  if (rc != MODE_OK) return rc;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const int ncols = F * tiles;
  hipLaunchKernelGGL(mvphoto_fwd_kernel, dim3(ncols), dim3(NT), 0, st, ref, src, depth, ps, S, H, W, tiles_w, tiles, p, win, slab);
  hipLaunchKernelGGL(mvphoto_final_kernel, dim3(1), dim3(NT), 0, st, slab, ncols, F, H, W, p, stats, loss);
  return mode::check_launch(who);
}

extern "C" int mode_mvphoto_loss_bwd(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                                     const mode_photometric_params* params, const unsigned char* win, const double* stats,
                                     const float* gloss, float* gdepth, mode_stream_t stream) {
  const char* who = "mode_mvphoto_loss_bwd";
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  MODE_REQUIRE(win && stats && gloss && gdepth, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  int rc = check_common(who, ref, src, depth, poses, S, F, H, W, params, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  hipLaunchKernelGGL(mvphoto_bwd_kernel, dim3(F * tiles), dim3(NT), 0, mode::as_stream(stream), ref, src, depth, ps, S, F, H, W, tiles_w,
                     tiles, p, win, stats, gloss, gdepth);
  return mode::check_launch(who);
}
